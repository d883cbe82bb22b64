// What the host side (uc_scene_api.cpp) and the kernel file (uc_scene_kernel.hip) of libuchirp_scene.so share.  The
// frame format and the call's geometry travel in the link simulator's Params (uc_link.hpp): n_streams is the number of
// microphones, text_stride the pitch of the transmissions' texts.
#pragma once
#include "uc_link.hpp"

namespace uc_scene_dev {

using uc_link_dev::Params;
using uc_link_dev::THREADS;
using uc_link_dev::TILE_QUADS;

// one path as the kernel reads it (40 bytes): what uc_link_dev::Stream holds for a stream, the sounding symbols of its
// transmission (2 + n_preamble + 8 * text_len) and where its text lies
struct Path {
  double rate;        // seconds of transmitter time per output sample: (1 / fs_out) * (1 + ppm * 1e-6)
  double t0;          // (origin * (1 + ppm * 1e-6) - lead_samples) / fs_out
  int64_t origin;     // the sample nearest to where the frame begins on the receiver's clock
  float amp;          // gain * sqrt 2
  uint32_t n_on;
  uint32_t tx;
  uint32_t pad;
};

// one microphone (16 bytes; the layout of uc_scene_mic)
struct Mic {
  uint32_t first_path;
  uint32_t n_paths;
  float sigma;
  uint32_t pad;
};

constexpr uint32_t MAX_PATHS = 16;

// workgroups of the kernel for `dtype` that one CU holds at once (the runtime's occupancy figure; <= 0: unknown)
int resident_blocks_per_cu(int dtype);

// launch (uc_scene_kernel.hip); dtype: UC_LINK_DTYPE_*; returns the hipError_t of the launch as int
int launch_render(int dtype, unsigned grid, void* stream, const Params& p, const Mic* mics, const Path* paths, const uint8_t* text,
                  void* out);

}  // namespace uc_scene_dev
