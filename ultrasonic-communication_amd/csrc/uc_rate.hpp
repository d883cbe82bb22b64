// What the host side (uc_rate_api.cpp) and the kernel file (uc_rate_kernel.hip) of libuchirp_rate.so share.
#pragma once
#include <cstddef>
#include <cstdint>

namespace uc_rate_dev {

constexpr int THREADS = 256;             // 4 waves; a lane is one output sample of the tile
constexpr int ROWS = 16;                 // rows of a unit: 8 pairs, a pair is one packed multiply-add
constexpr int WINDOW = 504;              // input samples of one row that a unit stages, at most (8 pairs x 505 x 8 B of LDS: 5 workgroups per CU)
constexpr int TAPS_MAX = 128;
constexpr uint32_t RATIO_MAX = 4096;

constexpr int DT_I16 = 0, DT_F32 = 1;    // UC_RATE_DTYPE_*

// Outputs of one tile: at most a lane each, and so few that the inputs under them fit the window.  The newest input of the
// tile's last output lies ((up - 1) + (n - 1) down) div up samples behind that of its first at most, and the oldest
// taps - 1 before it: (n - 1) down <= (WINDOW - taps) up keeps the sum within WINDOW.  taps <= 128 and
// down / up < 16 (what taps <= 128 leaves at half >= 4) give at least 24.
constexpr uint32_t tile_outputs(uint32_t up, uint32_t down, uint32_t taps) {
  const uint64_t n = 1 + (uint64_t)(WINDOW - taps) * up / down;
  return n < (uint64_t)THREADS ? (uint32_t)n : (uint32_t)THREADS;
}

struct Params {
  const void* in;
  float* out;
  const float* table;        // D[j][f] = C[p(f)][j] at table[j * up + f], f = m mod up: the table by output phase, transposed
  int64_t in_first;          // absolute sample of element 0 of every input row
  int64_t n_in;
  int64_t out_first;
  int64_t n_out;
  uint64_t in_stride;
  uint64_t out_stride;
  uint32_t tiles_per_row;    // ceil(n_out / tile), below 2^31
  uint32_t row_blocks;       // ceil(n_rows / ROWS)
  uint32_t n_rows;
  uint32_t up, down, taps, centre;
  uint32_t tile;             // tile_outputs(up, down, taps)
};

// workgroups of the kernel for `dtype` that one CU holds at once (the runtime's occupancy figure; <= 0: unknown)
int resident_blocks_per_cu(int dtype);

// launch (uc_rate_kernel.hip); dtype: UC_RATE_DTYPE_*; returns the hipError_t of the launch as int
int launch_convert(int dtype, unsigned grid, void* stream, const Params& p);

}  // namespace uc_rate_dev
