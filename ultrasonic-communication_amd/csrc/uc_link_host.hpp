// uc_link_host.hpp -- what the C-ABI files of libuchirp_link.so (uc_link_api.cpp) and libuchirp_scene.so
// (uc_scene_api.cpp) share on top of uc_host.hpp: the checks and defaults of the frame format and of the output formats.
// The RESTRICTION of uc_host.hpp (one including translation unit per library) holds for this header too.
#pragma once
#include "uc_host.hpp"

#include "../../include/uchirp_link.h"

namespace {

bool is_device_ptr(const void* p) { return device_of(p) >= 0; }

size_t elem_size(int dtype) {
  switch (dtype) {
    case UC_LINK_DTYPE_I32:
    case UC_LINK_DTYPE_F32: return 4;
    case UC_LINK_DTYPE_I16: return 2;
    default: return 0;
  }
}

bool config_ok(const uc_link_config* c) {
  if (!(c->fs_tx > 0.0) || !(c->t_symbol > 0.0) || !std::isfinite(c->fs_tx) || !std::isfinite(c->t_symbol)) return false;
  if (!std::isfinite(c->f0) || !std::isfinite(c->f1)) return false;
  const double n = c->t_symbol * c->fs_tx;
  return n >= 2.0 && n < 1e9 && c->n_preamble < (1u << 20) && c->n_guard < (1u << 20);
}

// the format of the reference transmission: 44100 Hz, 0.0262 s, 16000 .. 19000 Hz, 7 preamble symbols, 12 guard symbols
void reference_config(uc_link_config* cfg) {
  memset(cfg, 0, sizeof(*cfg));
  cfg->fs_tx = 44100.0;
  cfg->t_symbol = 0.0262;
  cfg->f0 = 16000.0;
  cfg->f1 = 19000.0;
  cfg->n_preamble = 7;
  cfg->n_guard = 12;
}

}  // namespace
