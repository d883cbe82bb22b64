// uc_iir_api.cpp -- the C-ABI of include/uchirp_iir.h on top of uc_iir_kernel.hip: the host function of the definition (one
// row of a cascade, on the arithmetic of uc_iir.hpp that the kernel compiles too), the coefficient sets, the checks that are
// its own, the launch.  The object's base, create and destroy, the staging of row_map and set_index and the checks of the row
// matrices are the shared host layer's (uc_host.hpp: header-only, nothing crosses a library boundary): libuchirp_iir.so
// stands alone.  No CPU compute path exists behind uc_iir_run: without a usable HIP device uc_iir_create fails.  Every entry
// point leaves the calling thread's current HIP device as it found it.
#include "../../include/uchirp_iir.h"
#include "uc_host.hpp"
#include "uc_iir.hpp"

using namespace uc_iir_dev;

static_assert(UC_IIR_DTYPE_I32 == DT_I32 && UC_IIR_DTYPE_F32 == DT_F32, "dtype values");
static_assert(UC_IIR_MAX_SECTIONS == MAX_SECTIONS && UC_IIR_MAX_SETS == MAX_SETS && UC_IIR_SECTION_WORDS == COEFS && UC_IIR_STATE_WORDS == STATE_WORDS,
              "constants of uchirp_iir.h");

struct uc_iir : HostBase {
  float* sections_dev = nullptr;   // MAX_SETS x MAX_SECTIONS x 5 floats; n_sets x n_sections x 5 of them in use
  uint32_t n_sets = 0;
  int n_sections = 0;
};

namespace {

int check_sections(const char* who, const float* sections, size_t n_sets, int n_sections) {
  if (!sections) return fail(-EINVAL, "%s: sections is NULL", who);
  if (n_sections < 1 || n_sections > MAX_SECTIONS) return fail(-EINVAL, "%s: n_sections %d not in 1 .. %d", who, n_sections, MAX_SECTIONS);
  if (n_sets < 1 || n_sets > (size_t)MAX_SETS) return fail(-EINVAL, "%s: n_sets %zu not in 1 .. %d", who, n_sets, MAX_SETS);
  const size_t n = n_sets * (size_t)n_sections * COEFS;
  for (size_t k = 0; k < n; ++k)
    if (!std::isfinite(sections[k]))
      return fail(-EINVAL, "%s: set %zu, section %zu: coefficient %zu is not finite", who, k / ((size_t)n_sections * COEFS), k / COEFS % (size_t)n_sections,
                  k % COEFS);
  return 0;
}

template <int DT, int NS>
void filter_row(const float* c, const uint32_t* in, size_t n, float* state, float* out) {
  float z[2 * NS];
  for (int k = 0; k < 2 * NS; ++k) z[k] = state[k];
  for (size_t i = 0; i < n; ++i) out[i] = filter_sample<NS>(c, z, sample_of<DT>(in[i]));
  for (int k = 0; k < 2 * NS; ++k) state[k] = z[k];
}

template <int DT>
void filter_row_sections(int n_sections, const float* c, const uint32_t* in, size_t n, float* state, float* out) {
  switch (n_sections) {
    case 1: filter_row<DT, 1>(c, in, n, state, out); break;
    case 2: filter_row<DT, 2>(c, in, n, state, out); break;
    case 3: filter_row<DT, 3>(c, in, n, state, out); break;
    case 4: filter_row<DT, 4>(c, in, n, state, out); break;
    case 5: filter_row<DT, 5>(c, in, n, state, out); break;
    case 6: filter_row<DT, 6>(c, in, n, state, out); break;
    case 7: filter_row<DT, 7>(c, in, n, state, out); break;
    default: filter_row<DT, 8>(c, in, n, state, out); break;
  }
}

bool on_16_bytes(const void* p, size_t stride) { return ((uintptr_t)p & 15u) == 0 && (stride & 3u) == 0; }

}  // namespace

extern "C" {

int uc_iir_abi_version(void) { return UC_IIR_ABI_VERSION; }

const char* uc_iir_last_error(void) { return g_err.c_str(); }

int uc_iir_filter_row(const float* sections, int n_sections, const void* in, int dtype, size_t n, float state[16], float* out) {
  static const char WHO[] = "uc_iir_filter_row";
  if (!in || !state || !out) return fail(-EINVAL, "uc_iir_filter_row: in, state or out is NULL");
  if (int rc = check_dtype(WHO, dtype)) return rc;
  if (n == 0) return fail(-EINVAL, "uc_iir_filter_row: n is 0");
  if (int rc = check_sections(WHO, sections, 1, n_sections)) return rc;
  if (dtype == DT_F32)
    filter_row_sections<DT_F32>(n_sections, sections, (const uint32_t*)in, n, state, out);
  else
    filter_row_sections<DT_I32>(n_sections, sections, (const uint32_t*)in, n, state, out);
  return 0;
}

int uc_iir_create(int device, uc_iir** out) {
  if (!out) return fail(-EINVAL, "uc_iir_create: out is NULL");
  *out = nullptr;
  DeviceGuard guard;
  uc_iir* l = nullptr;
  int rc = open("uc_iir_create", "UC_IIR_GRID", device, &l);
  if (rc) return rc;
  hipError_t e = hipMalloc((void**)&l->sections_dev, (size_t)MAX_SETS * MAX_SECTIONS * COEFS * sizeof(float));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    l->sections_dev = nullptr;
    close_base(l);
    delete l;
    return fail(-ENOMEM, "uc_iir_create: the coefficient sets: %s", hipGetErrorString(e));
  }
  *out = l;
  return 0;
}

void uc_iir_destroy(uc_iir* l) {
  if (!l) return;
  DeviceGuard guard;
  close_base(l);
  (void)hipDeviceSynchronize();      // a call that staged nothing left no event to wait for
  if (l->sections_dev) (void)hipFree(l->sections_dev);
  delete l;
}

int uc_iir_set_sections(uc_iir* l, const float* sections, size_t n_sets, int n_sections) {
  static const char WHO[] = "uc_iir_set_sections";
  if (!l) return fail(-EINVAL, "uc_iir_set_sections: iir is NULL");
  if (int rc = check_sections(WHO, sections, n_sets, n_sections)) return rc;
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(e, WHO, "hipDeviceSynchronize");   // no launch may still read the old sets
  if ((e = hipMemcpy(l->sections_dev, sections, n_sets * (size_t)n_sections * COEFS * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess)
    return hip_fail(e, WHO, "hipMemcpy");
  l->n_sets = (uint32_t)n_sets;
  l->n_sections = n_sections;
  return 0;
}

int uc_iir_run(uc_iir* l, const void* in_dev, int in_dtype, size_t n_in_rows, size_t in_stride, size_t n_rows, size_t n_samples,
               const uint32_t* row_map, const uint32_t* set_index, float* state_dev, float* out_dev, size_t out_stride, void* hip_stream) {
  static const char WHO[] = "uc_iir_run";
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_iir_run: iir is NULL");
  if (!in_dev || !state_dev || !out_dev) return fail(-EINVAL, "uc_iir_run: in_dev, state_dev or out_dev is NULL");
  if (int rc = check_dtype(WHO, in_dtype)) return rc;
  if (int rc = check_count(WHO, "n_in_rows", n_in_rows)) return rc;
  if (int rc = check_count(WHO, "n_rows", n_rows)) return rc;
  if (n_samples == 0) return fail(-EINVAL, "uc_iir_run: n_samples is 0");
  if (int rc = check_stride(WHO, "in_stride", in_stride, "n_samples", n_samples)) return rc;
  if (int rc = check_stride(WHO, "out_stride", out_stride, "n_samples", n_samples)) return rc;
  const size_t istride = stride_or(in_stride, n_samples), ostride = stride_or(out_stride, n_samples);
  if (int rc = check_strides_max(WHO, istride, ostride)) return rc;
  if (int rc = check_extent(WHO, n_in_rows, istride, n_rows, ostride, 1ull << 58, "n_rows * out_stride")) return rc;
  if ((((uintptr_t)in_dev | (uintptr_t)state_dev | (uintptr_t)out_dev) & 3u) != 0)
    return fail(-EINVAL, "uc_iir_run: in_dev, state_dev or out_dev is not a multiple of 4");
  const size_t in_bytes = span_bytes(n_in_rows, istride, n_samples, 4), out_bytes = span_bytes(n_rows, ostride, n_samples, 4);
  const size_t state_bytes = n_rows * STATE_WORDS * sizeof(float);
  if (int rc = check_disjoint(WHO, "out_dev", out_dev, out_bytes, "in_dev", in_dev, in_bytes)) return rc;
  if (int rc = check_disjoint(WHO, "state_dev", state_dev, state_bytes, "in_dev", in_dev, in_bytes)) return rc;
  if (int rc = check_disjoint(WHO, "state_dev", state_dev, state_bytes, "out_dev", out_dev, out_bytes)) return rc;
  if (l->n_sets == 0) return fail(-EINVAL, "uc_iir_run: no coefficient sets: call uc_iir_set_sections first");
  if (!row_map && n_rows > n_in_rows) return fail(-EINVAL, "uc_iir_run: n_rows %zu > n_in_rows %zu without a row_map", n_rows, n_in_rows);
  if (row_map)
    for (size_t r = 0; r < n_rows; ++r)
      if (row_map[r] >= n_in_rows) return fail(-EINVAL, "uc_iir_run: row_map[%zu] = %u; n_in_rows %zu", r, row_map[r], n_in_rows);
  if (set_index)
    for (size_t r = 0; r < n_rows; ++r)
      if (set_index[r] >= l->n_sets) return fail(-EINVAL, "uc_iir_run: set_index[%zu] = %u; %u sets", r, set_index[r], l->n_sets);
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if (int rc = check_on_device(WHO, "in_dev", in_dev, l->device)) return rc;
  if (int rc = check_on_device(WHO, "state_dev", state_dev, l->device)) return rc;
  if (int rc = check_on_device(WHO, "out_dev", out_dev, l->device)) return rc;
  // the two host arrays travel through the staging pair, row_map first; a call without them stages nothing
  const size_t words = ((row_map ? 1 : 0) + (set_index ? 1 : 0)) * n_rows, bytes = words * sizeof(uint32_t);
  StagingSlot* sl = nullptr;
  if (bytes)
    if (int rc = stage_begin(l, bytes, WHO, &sl)) return rc;

  // ---- stage
  Params p;
  memset(&p, 0, sizeof(p));
  if (sl) {
    uint32_t* host = (uint32_t*)sl->pinned;
    const uint32_t* dev = (const uint32_t*)sl->dev;
    if (row_map) {
      memcpy(host, row_map, n_rows * sizeof(uint32_t));
      p.row_map = dev;
      host += n_rows;
      dev += n_rows;
    }
    if (set_index) {
      memcpy(host, set_index, n_rows * sizeof(uint32_t));
      p.set_index = dev;
    }
  }
  p.in = in_dev;
  p.out = out_dev;
  p.state = state_dev;
  p.sections = l->sections_dev;
  p.in_stride = istride;
  p.out_stride = ostride;
  p.n_samples = n_samples;
  p.n_rows = (uint32_t)n_rows;
  p.row_blocks = (uint32_t)((n_rows + LANES - 1) / LANES);
  // a single row has no second row for its stride to misplace
  p.in_vec = on_16_bytes(in_dev, n_in_rows > 1 ? istride : 0) ? 1u : 0u;
  p.out_vec = on_16_bytes(out_dev, n_rows > 1 ? ostride : 0) ? 1u : 0u;
  // one one-wave workgroup per 64 rows; UC_IIR_GRID (under UC_TUNING=1) makes fewer of them walk the row blocks
  unsigned grid = p.row_blocks;
  if (l->grid_override && l->grid_override < grid) grid = l->grid_override;

  // ---- enqueue
  hipStream_t hs = (hipStream_t)hip_stream;
  if (sl)
    if (int rc = stage_copy(sl, bytes, hs, WHO)) return rc;
  e = (hipError_t)launch_filter(in_dtype, l->n_sections, grid, hs, p);
  if (sl) return stage_end(l, sl, hs, e, WHO);
  if (e != hipSuccess) return hip_fail(e, WHO, "launch");
  return 0;
}

}  // extern "C"
