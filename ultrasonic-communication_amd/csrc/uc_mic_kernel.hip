// uc_mic_kernel.hip -- the microphone model's kernel (gfx950): every input row (float or DFSDM words at 78 125 Hz) becomes
// the 1-bit PDM stream of a MEMS microphone, 32 bits per sample, packed as uc_dfsdm_sinc5 reads them.  include/uchirp_mic.h
// states the definition; uchirp/mic.py holds it in numpy integers (`model`); uc_mic.hpp holds the arithmetic itself, shared
// with uc_mic_modulate_row.
//
// The modulator is a nonlinear recurrence: bit t needs the integrators of bit t - 1, so a row cannot be cut in time.  The
// parallel axis is the rows: a lane is one row, a wave 64 rows, a workgroup ONE wave, so that 1024 workgroups (65 536
// microphones) are one wave on each of the chip's 1024 SIMDs.  A lane reads its row's state once, walks the row and writes
// the state once.
//
// Memory.  A lane that loads 16 bytes of its own row makes every load instruction touch 64 different lines, and a line is
// visited eight times, thousands of cycles apart; measured that way the chip fetched 3.5 times the input's bytes and wrote
// 2.0 times the output's (profiles/r18_mic.txt).  So, where both matrices put every row on 16 bytes, the wave moves TILES
// of 64 rows x 16 samples through LDS: four lanes load the 64 contiguous bytes of one row, 16 rows per instruction, the next
// tile's four loads in flight while the 512 bit-steps of this one run; every lane then reads its own row's 16 samples from
// LDS, and the 16 words go back the same way.  Rows in LDS lie 20 words apart, so that the 16-byte accesses of 16 lanes to
// their own rows fall on 64 different banks.  What is left behind the last whole tile -- and the whole row where a pointer
// or a stride does not put the rows on 16 bytes -- goes DIRECT: groups of four samples as one 16-byte access where the
// matrix allows it and as four dwords where not, the next group's load in flight; the up to three samples behind the last
// group as dwords.
//
// All arithmetic is int32 with wrap-around (unsigned in the code), so the bits depend on the row's samples and its state
// only, never on the path or the grid: row blocks are dealt blockIdx.x, + gridDim.x, ...
#include <hip/hip_runtime.h>

#include "uc_mic.hpp"

namespace uc_mic_dev {
namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

constexpr int TILE = 16;                 // samples of a row in one staged tile: 64 bytes, four 16-byte pieces
constexpr int PITCH = 5;                 // 16-byte units between two rows of a tile in LDS: four pieces and one of padding
constexpr int SWEEPS = LANES / 16;       // a load instruction covers 16 rows (4 lanes a row): 4 of them cover the tile

template <int DT>
__device__ __forceinline__ int32_t quantise(uint32_t raw, float scale) {
  return DT == DT_F32 ? quantise_f32(__uint_as_float(raw), scale) : quantise_i32((int32_t)raw);
}

template <int DT>
__device__ __forceinline__ u4 modulate_group(State& s, u4 x, float scale) {
  u4 w;
  w.x = modulate_sample(s, quantise<DT>(x.x, scale));
  w.y = modulate_sample(s, quantise<DT>(x.y, scale));
  w.z = modulate_sample(s, quantise<DT>(x.z, scale));
  w.w = modulate_sample(s, quantise<DT>(x.w, scale));
  return w;
}

// four samples of a row from element j on (all four exist); `vec` is uniform
__device__ __forceinline__ u4 load_group(const uint32_t* row, uint64_t j, bool vec) {
  if (vec) return *reinterpret_cast<const u4*>(row + j);
  u4 v;
  v.x = row[j];
  v.y = row[j + 1];
  v.z = row[j + 2];
  v.w = row[j + 3];
  return v;
}

__device__ __forceinline__ void store_group(uint32_t* row, uint64_t j, bool vec, u4 w) {
  if (vec) {
    *reinterpret_cast<u4*>(row + j) = w;
    return;
  }
  row[j] = w.x;
  row[j + 1] = w.y;
  row[j + 2] = w.z;
  row[j + 3] = w.w;
}

template <int DT>
__global__ __launch_bounds__(LANES) void mic_kernel(const Params p) {
  __shared__ u4 tile_in[LANES * PITCH], tile_out[LANES * PITCH];
  const bool in_vec = p.in_vec != 0, out_vec = p.out_vec != 0;
  const uint32_t lane = threadIdx.x;
  const uint32_t piece = lane & 3u, sub = lane >> 2;                // of the tile's moves: lane = (row sub + 16 k, piece)
  const uint64_t tiles = in_vec && out_vec ? p.n_samples / TILE : 0;
  for (uint32_t rb = blockIdx.x; rb < p.row_blocks; rb += gridDim.x) {
    const uint64_t row0 = (uint64_t)rb * LANES;
    const uint64_t r = row0 + lane;
    const bool live = r < p.n_rows;                                 // (a lane without a row goes along through the tiles with zeros)
    const uint32_t* const in = (const uint32_t*)p.in + r * p.in_stride;
    uint32_t* const out = p.out + r * p.out_stride;
    int32_t* const st = p.state + r * 4;
    State s = {0, 0, 0};
    if (live) s = {(uint32_t)st[0], (uint32_t)st[1], (uint32_t)st[2]};   // (dwords: once per row, and any alignment will do)

    // ---- whole tiles through LDS
    if (tiles) {
      const uint32_t* src[SWEEPS];
      uint32_t* dst[SWEEPS];
      bool there[SWEEPS];
      u4 nxt[SWEEPS];
#pragma unroll
      for (int k = 0; k < SWEEPS; ++k) {
        const uint64_t row = row0 + sub + 16 * k;
        there[k] = row < p.n_rows;
        src[k] = (const uint32_t*)p.in + (there[k] ? row : 0) * p.in_stride + piece * 4;
        dst[k] = p.out + (there[k] ? row : 0) * p.out_stride + piece * 4;
        nxt[k] = u4{0, 0, 0, 0};
        if (there[k]) nxt[k] = *reinterpret_cast<const u4*>(src[k]);
      }
      for (uint64_t t = 0; t < tiles; ++t) {
#pragma unroll
        for (int k = 0; k < SWEEPS; ++k) tile_in[(sub + 16 * k) * PITCH + piece] = nxt[k];
        __syncthreads();                                            // (one wave: the wait for LDS; tile_out of the last pass is read)
        if (t + 1 < tiles) {
#pragma unroll
          for (int k = 0; k < SWEEPS; ++k)
            if (there[k]) nxt[k] = *reinterpret_cast<const u4*>(src[k] + (t + 1) * TILE);
        }
#pragma unroll
        for (int g = 0; g < TILE / GROUP; ++g) tile_out[lane * PITCH + g] = modulate_group<DT>(s, tile_in[lane * PITCH + g], p.scale);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SWEEPS; ++k)
          if (there[k]) *reinterpret_cast<u4*>(dst[k] + t * TILE) = tile_out[(sub + 16 * k) * PITCH + piece];
      }
    }
    if (!live) continue;                                            // (no barrier below)

    // ---- the rest of the row (all of it where the matrices do not allow the tiles), direct
    const uint64_t first = tiles * TILE;
    const uint64_t whole = first + ((p.n_samples - first) & ~(uint64_t)(GROUP - 1));   // the end of the last whole group
    u4 cur = {0, 0, 0, 0};
    if (first < whole) cur = load_group(in, first, in_vec);
    for (uint64_t j = first; j < whole; j += GROUP) {
      u4 nxt = {0, 0, 0, 0};
      if (j + GROUP < whole) nxt = load_group(in, j + GROUP, in_vec);
      store_group(out, j, out_vec, modulate_group<DT>(s, cur, p.scale));
      cur = nxt;
    }
    for (uint64_t j = whole; j < p.n_samples; ++j) out[j] = modulate_sample(s, quantise<DT>(in[j], p.scale));
    st[0] = (int32_t)s.prev;
    st[1] = (int32_t)s.s1;
    st[2] = (int32_t)s.s2;
    st[3] = 0;
  }
}

}  // namespace

int launch_modulate(int dtype, unsigned grid, void* stream, const Params& p) {
  hipStream_t hs = (hipStream_t)stream;
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL(mic_kernel<DT_F32>, dim3(grid), dim3(LANES), 0, hs, p); break;
    case DT_I32: hipLaunchKernelGGL(mic_kernel<DT_I32>, dim3(grid), dim3(LANES), 0, hs, p); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

}  // namespace uc_mic_dev
