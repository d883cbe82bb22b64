// uc_scene_api.cpp -- the C-ABI of include/uchirp_scene.h on top of uc_scene_kernel.hip: the scene object and its frame
// format, the checks and the staging that are its own, the launch.  The object's base, create and destroy, the staging
// protocol, the grid and the checks of the row matrices are the shared host layer's (uc_host.hpp: header-only, nothing
// crosses a library boundary); the frame format's checks are uc_link_host.hpp's, shared with uc_link_api.cpp at no symbol:
// libuchirp_scene.so stands alone.  No CPU compute path exists here: without a usable HIP device uc_scene_create fails.
// Every entry point leaves the calling thread's current HIP device as it found it.
#include "../../include/uchirp_scene.h"
#include "uc_link_host.hpp"
#include "uc_scene.hpp"

using namespace uc_scene_dev;

// staging: [n_paths Path records][n_mics Mic records][n_tx * text_stride bytes]
struct uc_scene : HostBase {
  uc_link_config cfg{};
  int n_sym = 0;
};

extern "C" {

int uc_scene_abi_version(void) { return UC_SCENE_ABI_VERSION; }

const char* uc_scene_last_error(void) { return g_err.c_str(); }

int uc_scene_default_config(uc_link_config* cfg) {
  if (!cfg) return fail(-EINVAL, "uc_scene_default_config: cfg is NULL");
  reference_config(cfg);
  return 0;
}

int uc_scene_create(int device, const uc_link_config* cfg, uc_scene** out) {
  if (!out) return fail(-EINVAL, "uc_scene_create: out is NULL");
  *out = nullptr;
  uc_link_config c;
  if (cfg)
    c = *cfg;
  else
    uc_scene_default_config(&c);
  if (!config_ok(&c)) return fail(-EINVAL, "uc_scene_create: not a frame format (fs_tx, t_symbol > 0, at least 2 samples per symbol)");
  DeviceGuard guard;
  const int rc = open("uc_scene_create", "UC_SCENE_GRID", device, out);
  if (rc) return rc;
  (*out)->cfg = c;
  (*out)->n_sym = (int)(c.t_symbol * c.fs_tx);
  return 0;
}

void uc_scene_destroy(uc_scene* l) {
  if (!l) return;
  DeviceGuard guard;
  close_base(l);
  delete l;
}

int uc_scene_render(uc_scene* l, const uint8_t* text, size_t text_stride, const uint32_t* text_len, size_t n_tx,
                    const uc_scene_path* paths, size_t n_paths, const uc_scene_mic* mics, size_t n_mics, void* out_dev, int dtype,
                    double fs_out, uint64_t first_sample, size_t n_samples, size_t stride_elems, uint64_t seed, void* hip_stream) {
  static const char WHO[] = "uc_scene_render";
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_scene_render: scene is NULL");
  if (!out_dev) return fail(-EINVAL, "uc_scene_render: out_dev is NULL");
  if (int rc = check_count(WHO, "n_mics", n_mics)) return rc;
  if (n_paths > 0xFFFFFFFFull || n_tx > 0xFFFFFFFFull) return fail(-EINVAL, "uc_scene_render: n_paths / n_tx out of range");
  if (!mics) return fail(-EINVAL, "uc_scene_render: mics is NULL");
  if (n_paths && !paths) return fail(-EINVAL, "uc_scene_render: paths is NULL, n_paths %zu", n_paths);
  if (n_tx && !text_len) return fail(-EINVAL, "uc_scene_render: text_len is NULL, n_tx %zu", n_tx);
  if (n_samples == 0) return fail(-EINVAL, "uc_scene_render: n_samples is 0");
  const size_t esz = elem_size(dtype);
  if (!esz) return fail(-EINVAL, "uc_scene_render: unknown dtype %d", dtype);
  if (!(fs_out > 0.0) || !std::isfinite(fs_out)) return fail(-EINVAL, "uc_scene_render: fs_out must be positive");
  if (text_stride > UC_LINK_MAX_TEXT) return fail(-EINVAL, "uc_scene_render: text_stride %zu > %d", text_stride, UC_LINK_MAX_TEXT);
  const size_t stride = stride_or(stride_elems, n_samples);
  if (int rc = check_stride(WHO, "stride_elems", stride_elems, "n_samples", n_samples)) return rc;
  // the reach: every sample index stays below 2^53, so its distance to a path's origin is exact in double (frame_time())
  if (first_sample > UC_LINK_MAX_FIRST_SAMPLE || n_samples > UC_LINK_MAX_SAMPLES)
    return fail(-EINVAL, "uc_scene_render: sample range too large (first_sample <= 2^52, n_samples <= 2^40)");
  bool any_text = false;
  for (size_t t = 0; t < n_tx; ++t) {
    if (text_len[t] > text_stride)
      return fail(-EINVAL, "uc_scene_render: transmission %zu: text_len %u > text_stride %zu", t, text_len[t], text_stride);
    any_text |= text_len[t] != 0;
  }
  if (any_text && !text) return fail(-EINVAL, "uc_scene_render: text is NULL");
  for (size_t k = 0; k < n_paths; ++k) {
    const uc_scene_path& q = paths[k];
    if (q.tx >= n_tx) return fail(-EINVAL, "uc_scene_render: path %zu: tx %u >= n_tx %zu", k, q.tx, n_tx);
    if (!std::isfinite(q.lead_samples) || !std::isfinite(q.gain) || !std::isfinite(q.ppm))
      return fail(-EINVAL, "uc_scene_render: path %zu: lead_samples, gain and ppm must be finite", k);
  }
  for (size_t m = 0; m < n_mics; ++m) {
    const uc_scene_mic& q = mics[m];
    if (q.n_paths > UC_SCENE_MAX_PATHS)
      return fail(-EINVAL, "uc_scene_render: microphone %zu: n_paths %u > %d", m, q.n_paths, UC_SCENE_MAX_PATHS);
    if ((uint64_t)q.first_path + q.n_paths > n_paths)
      return fail(-EINVAL, "uc_scene_render: microphone %zu: paths [%u, %u + %u) beyond n_paths %zu", m, q.first_path, q.first_path,
                  q.n_paths, n_paths);
    if (!std::isfinite(q.sigma) || q.sigma < 0.0f) return fail(-EINVAL, "uc_scene_render: microphone %zu: sigma must be finite and >= 0", m);
  }
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if (!is_device_ptr(out_dev)) return fail(-EINVAL, "uc_scene_render: out_dev is not device memory");
  const uint64_t first_quad = first_sample / 4, end_quad = (first_sample + n_samples + 3) / 4;
  const uint64_t tiles_per_mic = (end_quad - first_quad + TILE_QUADS - 1) / TILE_QUADS;
  const size_t path_bytes = n_paths * sizeof(Path), mic_bytes = n_mics * sizeof(Mic);
  const size_t bytes = path_bytes + mic_bytes + n_tx * text_stride;
  StagingSlot* sl;
  if (int rc = stage_begin(l, bytes, WHO, &sl)) return rc;

  // ---- stage
  const uc_link_config& c = l->cfg;
  Path* prec = (Path*)sl->pinned;
  for (size_t k = 0; k < n_paths; ++k) {
    const uc_scene_path& q = paths[k];
    const FrameOrigin fo = frame_origin(q.lead_samples, q.ppm, fs_out);
    prec[k].rate = fo.rate;
    prec[k].t0 = fo.t0;
    prec[k].origin = fo.origin;
    prec[k].amp = (float)((double)q.gain * 1.4142135623730951);
    prec[k].n_on = 2u + c.n_preamble + 8u * text_len[q.tx];
    prec[k].tx = q.tx;
    prec[k].pad = 0;
  }
  Mic* mrec = (Mic*)((char*)sl->pinned + path_bytes);
  for (size_t m = 0; m < n_mics; ++m) {
    mrec[m].first_path = mics[m].first_path;
    mrec[m].n_paths = mics[m].n_paths;
    mrec[m].sigma = mics[m].sigma;
    mrec[m].pad = 0;
  }
  if (n_tx * text_stride) {
    if (text)
      memcpy((char*)sl->pinned + path_bytes + mic_bytes, text, n_tx * text_stride);
    else
      memset((char*)sl->pinned + path_bytes + mic_bytes, 0, n_tx * text_stride);
  }
  Params p;
  memset(&p, 0, sizeof(p));
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
  p.tiles_per_stream = (uint32_t)tiles_per_mic;
  p.n_preamble = c.n_preamble;
  p.text_stride = (uint32_t)text_stride;
  p.n_streams = (uint32_t)n_mics;
  // the scene kernels' scalar registers leave 7 workgroups of 4 waves per CU where the link kernel has 8
  const uint64_t grid = persistent_grid(l, dtype, resident_blocks_per_cu, 7, (uint64_t)n_mics * tiles_per_mic);

  // ---- enqueue
  hipStream_t hs = (hipStream_t)hip_stream;
  if (int rc = stage_copy(sl, bytes, hs, WHO)) return rc;
  const char* d = (const char*)sl->dev;
  e = (hipError_t)launch_render(dtype, (unsigned)grid, hs, p, (const Mic*)(d + path_bytes), (const Path*)d,
                                (const uint8_t*)(d + path_bytes + mic_bytes), out_dev);
  return stage_end(l, sl, hs, e, WHO);
}

}  // extern "C"
