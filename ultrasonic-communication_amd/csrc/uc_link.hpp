// What the host side (uc_link_api.cpp) and the kernel file (uc_link_kernel.hip) of libuchirp_link.so share.
#pragma once
#include <cstddef>
#include <cstdint>

namespace uc_link_dev {

// one stream as the kernel reads it (40 bytes).  rate, t0 and origin are frame_origin()'s (uc_link_host.hpp): the seconds
// since the frame began at absolute sample j are (j - origin) * rate + t0, an integer difference and a time under a sample
struct Stream {
  double rate;        // seconds of transmitter time per output sample: (1 / fs_out) * (1 + ppm * 1e-6)
  double t0;          // (origin * (1 + ppm * 1e-6) - lead_samples) / fs_out: the frame's time at sample `origin`
  int64_t origin;     // the sample nearest to where the frame begins on the receiver's clock
  float amp;          // amplitude * sqrt 2
  float sigma;
  uint32_t text_len;
  uint32_t pad;
};

// the frame format and the call's geometry (by value)
struct Params {
  double sym_dur, inv_sym_dur;   // n_sym / fs_tx and its reciprocal
  double t_scale;                // fs_tx * t_symbol / (n_sym - 1): transmitter-clock seconds -> the law's t
  double f0, f1, half_k;         // half_k = (f1 - f0) / t_symbol / 2
  uint64_t first_sample, n_samples, stride;
  uint64_t seed;
  uint64_t first_quad;           // first_sample / 4
  uint32_t tiles_per_stream;     // tiles of TILE_QUADS Philox counters that cover one stream's samples
  uint32_t n_preamble;
  uint32_t text_stride;
  uint32_t n_streams;
};

constexpr int THREADS = 256;         // 4 waves; a wave owns 256 consecutive samples of one stream
constexpr int TILE_QUADS = THREADS;  // one lane = one Philox counter = 4 samples

// launches (uc_link_kernel.hip); dtype: UC_LINK_DTYPE_*; return the hipError_t of the launch as int
int launch_transmit(int dtype, unsigned grid, void* stream, const Params& p, const Stream* streams, const uint8_t* text, void* out);
int launch_words(unsigned grid, void* stream, uint64_t seed, uint64_t sid, uint64_t first_counter, uint64_t n_counters, uint32_t* out);

}  // namespace uc_link_dev
