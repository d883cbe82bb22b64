// uc_link_api.cpp -- the C-ABI of include/uchirp_link.h on top of uc_link_kernel.hip: the link object and its frame
// format, the checks and the staging that are its own, the two launches.  The object's base, create and destroy, the
// staging protocol, the grid and the checks of the row matrices are the shared host layer's (uc_host.hpp: header-only,
// nothing crosses a library boundary); the frame format's checks are uc_link_host.hpp's: libuchirp_link.so stands alone.
// No CPU compute path exists here: without a usable HIP device uc_link_create fails.  Every entry point leaves the calling
// thread's current HIP device as it found it.
#include "../../include/uchirp_link.h"
#include "uc_link.hpp"
#include "uc_link_host.hpp"

using namespace uc_link_dev;

// staging: [n_streams Stream records][n_streams * text_stride bytes]
struct uc_link : HostBase {
  uc_link_config cfg{};
  int n_sym = 0;
};

extern "C" {

int uc_link_abi_version(void) { return UC_LINK_ABI_VERSION; }

const char* uc_link_last_error(void) { return g_err.c_str(); }

int uc_link_default_config(uc_link_config* cfg) {
  if (!cfg) return fail(-EINVAL, "uc_link_default_config: cfg is NULL");
  reference_config(cfg);
  return 0;
}

int uc_link_frame_origin(double lead_samples, float ppm, double fs_out, uc_link_origin* out) {
  if (!out) return fail(-EINVAL, "uc_link_frame_origin: out is NULL");
  if (!std::isfinite(lead_samples) || !std::isfinite(ppm)) return fail(-EINVAL, "uc_link_frame_origin: lead_samples and ppm must be finite");
  if (!(fs_out > 0.0) || !std::isfinite(fs_out)) return fail(-EINVAL, "uc_link_frame_origin: fs_out must be positive");
  const FrameOrigin fo = frame_origin(lead_samples, ppm, fs_out);
  out->origin = fo.origin;
  out->t0 = fo.t0;
  out->rate = fo.rate;
  return 0;
}

int uc_link_create(int device, const uc_link_config* cfg, uc_link** out) {
  if (!out) return fail(-EINVAL, "uc_link_create: out is NULL");
  *out = nullptr;
  uc_link_config c;
  if (cfg)
    c = *cfg;
  else
    uc_link_default_config(&c);
  if (!config_ok(&c)) return fail(-EINVAL, "uc_link_create: not a frame format (fs_tx, t_symbol > 0, at least 2 samples per symbol)");
  DeviceGuard guard;
  const int rc = open("uc_link_create", "UC_LINK_GRID", device, out);
  if (rc) return rc;
  (*out)->cfg = c;
  (*out)->n_sym = (int)(c.t_symbol * c.fs_tx);
  return 0;
}

void uc_link_destroy(uc_link* l) {
  if (!l) return;
  DeviceGuard guard;
  close_base(l);
  delete l;
}

int uc_link_transmit(uc_link* l, const uint8_t* text, size_t text_stride, const uc_link_stream* params, size_t n_streams,
                     void* out_dev, int dtype, double fs_out, uint64_t first_sample, size_t n_samples, size_t stride_elems,
                     uint64_t seed, void* hip_stream) {
  static const char WHO[] = "uc_link_transmit";
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_link_transmit: link is NULL");
  if (!params || !out_dev) return fail(-EINVAL, "uc_link_transmit: params / out_dev is NULL");
  if (int rc = check_count(WHO, "n_streams", n_streams)) return rc;
  if (n_samples == 0) return fail(-EINVAL, "uc_link_transmit: n_samples is 0");
  const size_t esz = elem_size(dtype);
  if (!esz) return fail(-EINVAL, "uc_link_transmit: unknown dtype %d", dtype);
  if (!(fs_out > 0.0) || !std::isfinite(fs_out)) return fail(-EINVAL, "uc_link_transmit: fs_out must be positive");
  if (text_stride > UC_LINK_MAX_TEXT) return fail(-EINVAL, "uc_link_transmit: text_stride %zu > %d", text_stride, UC_LINK_MAX_TEXT);
  const size_t stride = stride_or(stride_elems, n_samples);
  if (int rc = check_stride(WHO, "stride_elems", stride_elems, "n_samples", n_samples)) return rc;
  // the reach: every sample index stays below 2^53, so its distance to a stream's origin is exact in double (frame_time())
  if (first_sample > UC_LINK_MAX_FIRST_SAMPLE || n_samples > UC_LINK_MAX_SAMPLES)
    return fail(-EINVAL, "uc_link_transmit: sample range too large (first_sample <= 2^52, n_samples <= 2^40)");
  bool any_text = false;
  for (size_t s = 0; s < n_streams; ++s) {
    const uc_link_stream& q = params[s];
    if (q.text_len > text_stride)
      return fail(-EINVAL, "uc_link_transmit: stream %zu: text_len %u > text_stride %zu", s, q.text_len, text_stride);
    if (!std::isfinite(q.lead_samples) || !std::isfinite(q.amplitude) || !std::isfinite(q.sigma) || !std::isfinite(q.ppm) || q.sigma < 0.0f)
      return fail(-EINVAL, "uc_link_transmit: stream %zu: parameters must be finite, sigma >= 0", s);
    any_text |= q.text_len != 0;
  }
  if (any_text && !text) return fail(-EINVAL, "uc_link_transmit: text is NULL");
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if (!is_device_ptr(out_dev)) return fail(-EINVAL, "uc_link_transmit: out_dev is not device memory");
  const uint64_t first_quad = first_sample / 4, end_quad = (first_sample + n_samples + 3) / 4;
  const uint64_t tiles_per_stream = (end_quad - first_quad + TILE_QUADS - 1) / TILE_QUADS;
  const size_t rec_bytes = n_streams * sizeof(Stream);
  const size_t bytes = rec_bytes + n_streams * text_stride;
  StagingSlot* sl;
  if (int rc = stage_begin(l, bytes, WHO, &sl)) return rc;

  // ---- stage
  Stream* rec = (Stream*)sl->pinned;
  for (size_t s = 0; s < n_streams; ++s) {
    const uc_link_stream& q = params[s];
    const FrameOrigin fo = frame_origin(q.lead_samples, q.ppm, fs_out);
    rec[s].rate = fo.rate;
    rec[s].t0 = fo.t0;
    rec[s].origin = fo.origin;
    rec[s].amp = (float)((double)q.amplitude * 1.4142135623730951);
    rec[s].sigma = q.sigma;
    rec[s].text_len = q.text_len;
    rec[s].pad = 0;
  }
  if (text_stride) {
    if (text)
      memcpy((char*)sl->pinned + rec_bytes, text, n_streams * text_stride);
    else
      memset((char*)sl->pinned + rec_bytes, 0, n_streams * text_stride);
  }
  Params p;
  memset(&p, 0, sizeof(p));
  const uc_link_config& c = l->cfg;
  p.sym_dur = (double)l->n_sym / c.fs_tx;
  p.inv_sym_dur = 1.0 / p.sym_dur;
  p.t_scale = c.fs_tx * c.t_symbol / (double)(l->n_sym - 1);
  p.f0 = c.f0;
  p.f1 = c.f1;
  p.half_k = (c.f1 - c.f0) / c.t_symbol / 2.0;
  p.first_sample = first_sample;
  p.n_samples = n_samples;
  p.stride = stride;
  p.seed = seed;
  p.first_quad = first_quad;
  p.tiles_per_stream = (uint32_t)tiles_per_stream;
  p.n_preamble = c.n_preamble;
  p.text_stride = (uint32_t)text_stride;
  p.n_streams = (uint32_t)n_streams;
  const uint64_t n_tiles = (uint64_t)n_streams * tiles_per_stream;
  uint64_t grid = (uint64_t)l->cus * 8;       // 8 workgroups of 4 waves per CU: every wave slot of the chip
  if (l->grid_override) grid = l->grid_override;
  if (grid > n_tiles) grid = n_tiles;

  // ---- enqueue
  hipStream_t hs = (hipStream_t)hip_stream;
  if (int rc = stage_copy(sl, bytes, hs, WHO)) return rc;
  e = (hipError_t)launch_transmit(dtype, (unsigned)grid, hs, p, (const Stream*)sl->dev, (const uint8_t*)sl->dev + rec_bytes, out_dev);
  return stage_end(l, sl, hs, e, WHO);
}

int uc_link_noise_words(uc_link* l, uint64_t seed, uint64_t stream, uint64_t first_counter, size_t n_counters, uint32_t* out_dev,
                        void* hip_stream) {
  if (!l) return fail(-EINVAL, "uc_link_noise_words: link is NULL");
  if (!out_dev) return fail(-EINVAL, "uc_link_noise_words: out_dev is NULL");
  if (n_counters == 0 || n_counters > (1ull << 40)) return fail(-EINVAL, "uc_link_noise_words: n_counters %zu out of range", n_counters);
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, "uc_link_noise_words", "hipSetDevice");
  if (!is_device_ptr(out_dev)) return fail(-EINVAL, "uc_link_noise_words: out_dev is not device memory");
  uint64_t grid = (n_counters + THREADS - 1) / THREADS;
  const uint64_t cap = (uint64_t)l->cus * 8;
  if (grid > cap) grid = cap;
  e = (hipError_t)launch_words((unsigned)grid, hip_stream, seed, stream, first_counter, n_counters, out_dev);
  if (e != hipSuccess) return hip_fail(e, "uc_link_noise_words", "launch");
  return 0;
}

}  // extern "C"
