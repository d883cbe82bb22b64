// uc_iir_kernel.hip -- the recursive filter bank's kernel (gfx950): every output row is one input row (float or DFSDM words)
// through a cascade of 1 .. 8 biquad sections in float32.  include/uchirp_iir.h states the definition; uchirp/iir.py holds it
// in numpy float32 (`emulate32`); uc_iir.hpp holds the arithmetic itself, shared with uc_iir_filter_row.
//
// A recurrence cannot be cut in time: sample t needs the state behind sample t - 1.  The parallel axis is the rows, as in
// uc_mic_kernel.hip: a lane is one output row, a wave 64 rows, a workgroup ONE wave, so that 1024 workgroups (65 536 rows)
// are one wave on each of the chip's 1024 SIMDs.  A lane reads its set's coefficients (5 floats a section) and its row's
// state (2 floats a section) once, keeps both in registers while it walks the row, and writes the state once.  The section
// count is a template argument: a cascade padded with an identity section would turn -0 into +0.
//
// Memory, as the microphone model's: where both matrices put every row on 16 bytes and the wave's rows read their own input
// rows (no row_map, or the identity on these 64 rows), the wave moves TILES of 64 rows x 16 samples through LDS: four lanes
// load the 64 contiguous bytes of one row, 16 rows per instruction, the next tile's four loads in flight while this tile's
// arithmetic runs; every lane then reads its own row's 16 samples from LDS, and the 16 outputs go back the same way.  Rows
// in LDS lie 20 words apart, so that the 16-byte accesses of 16 lanes to their own rows fall on 64 different banks.  What is
// left behind the last whole tile -- and the whole row where a pointer or a stride does not put the rows on 16 bytes, or
// where row_map sends a row of the wave elsewhere -- goes DIRECT: groups of four samples as one 16-byte access where the
// matrix allows it and as four dwords where not, the next group's load in flight; the up to three samples behind the last
// group as dwords.
//
// The arithmetic is float32 without contraction and with denormals kept (uc_iir.hpp), one operation after the other in
// the order of the definition, so the bits depend on the row's samples, its state and its set only, never on the path or the
// grid: row blocks are dealt blockIdx.x, + gridDim.x, ...
#include <hip/hip_runtime.h>

#include "uc_iir.hpp"

namespace uc_iir_dev {
namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

constexpr int TILE = 16;                 // samples of a row in one staged tile: 64 bytes, four 16-byte pieces
constexpr int PITCH = 5;                 // 16-byte units between two rows of a tile in LDS: four pieces and one of padding
constexpr int SWEEPS = LANES / 16;       // a load instruction covers 16 rows (4 lanes a row): 4 of them cover the tile

template <int DT, int NS>
__device__ __forceinline__ uint32_t filter_word(const float* c, float* z, uint32_t raw) {
  return float_to_bits(filter_sample<NS>(c, z, sample_of<DT>(raw)));
}

template <int DT, int NS>
__device__ __forceinline__ u4 filter_group(const float* c, float* z, u4 x) {
  u4 w;
  w.x = filter_word<DT, NS>(c, z, x.x);
  w.y = filter_word<DT, NS>(c, z, x.y);
  w.z = filter_word<DT, NS>(c, z, x.z);
  w.w = filter_word<DT, NS>(c, z, x.w);
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

template <int DT, int NS>
__global__ __launch_bounds__(LANES) __attribute__((amdgpu_waves_per_eu(4, 4))) void iir_kernel(const Params p) {
  __shared__ u4 tile_in[LANES * PITCH], tile_out[LANES * PITCH];
  const bool in_vec = p.in_vec != 0, out_vec = p.out_vec != 0;
  const uint32_t lane = threadIdx.x;
  const uint32_t piece = lane & 3u, sub = lane >> 2;                // of the tile's moves: lane = (row sub + 16 k, piece)
  for (uint32_t rb = blockIdx.x; rb < p.row_blocks; rb += gridDim.x) {
    const uint64_t row0 = (uint64_t)rb * LANES;
    const uint64_t r = row0 + lane;
    const bool live = r < p.n_rows;                                 // (a lane without a row goes along through the tiles with zeros)
    const uint64_t src_row = live && p.row_map ? p.row_map[r] : r;
    // tiles: only where every row of the wave reads its own input row
    const bool own = p.row_map == nullptr || __all(src_row == r);
    const uint64_t tiles = in_vec && out_vec && own ? p.n_samples / TILE : 0;
    const uint32_t* const in = (const uint32_t*)p.in + src_row * p.in_stride;
    uint32_t* const out = (uint32_t*)p.out + r * p.out_stride;
    float* const st = p.state + r * STATE_WORDS;
    float c[COEFS * NS], z[2 * NS];
    const float* const mine = p.sections + (uint64_t)(live && p.set_index ? p.set_index[r] : 0u) * (COEFS * NS);
#pragma unroll
    for (int k = 0; k < COEFS * NS; ++k) c[k] = mine[k];
#pragma unroll
    for (int k = 0; k < 2 * NS; ++k) z[k] = live ? st[k] : 0.0f;     // (dwords: once per row, and any alignment will do)

    // ---- whole tiles through LDS
    if (tiles) {
      // sweep k moves row row0 + sub + 16 k: one pointer per matrix and 16 strides (uniform) from sweep to sweep
      const uint32_t* const src0 = (const uint32_t*)p.in + (row0 + sub) * p.in_stride + piece * 4;
      uint32_t* const dst0 = (uint32_t*)p.out + (row0 + sub) * p.out_stride + piece * 4;
      const uint64_t in_step = 16 * p.in_stride, out_step = 16 * p.out_stride;
      bool there[SWEEPS];
      u4 nxt[SWEEPS];
#pragma unroll
      for (int k = 0; k < SWEEPS; ++k) {
        there[k] = row0 + sub + 16 * k < p.n_rows;
        nxt[k] = u4{0, 0, 0, 0};
        if (there[k]) nxt[k] = *reinterpret_cast<const u4*>(src0 + k * in_step);
      }
      for (uint64_t t = 0; t < tiles; ++t) {
#pragma unroll
        for (int k = 0; k < SWEEPS; ++k) tile_in[(sub + 16 * k) * PITCH + piece] = nxt[k];
        __syncthreads();                                            // (one wave: the wait for LDS; tile_out of the last pass is read)
        if (t + 1 < tiles) {
#pragma unroll
          for (int k = 0; k < SWEEPS; ++k)
            if (there[k]) nxt[k] = *reinterpret_cast<const u4*>(src0 + k * in_step + (t + 1) * TILE);
        }
#pragma unroll 1
        for (int g = 0; g < TILE / GROUP; ++g) tile_out[lane * PITCH + g] = filter_group<DT, NS>(c, z, tile_in[lane * PITCH + g]);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SWEEPS; ++k)
          if (there[k]) *reinterpret_cast<u4*>(dst0 + k * out_step + t * TILE) = tile_out[(sub + 16 * k) * PITCH + piece];
      }
    }
    if (!live) continue;                                            // (no barrier below)

    // ---- the rest of the row (all of it where the matrices or row_map do not allow the tiles), direct
    const uint64_t first = tiles * TILE;
    const uint64_t whole = first + ((p.n_samples - first) & ~(uint64_t)(GROUP - 1));   // the end of the last whole group
    u4 cur = {0, 0, 0, 0};
    if (first < whole) cur = load_group(in, first, in_vec);
    for (uint64_t j = first; j < whole; j += GROUP) {
      u4 nxt = {0, 0, 0, 0};
      if (j + GROUP < whole) nxt = load_group(in, j + GROUP, in_vec);
      store_group(out, j, out_vec, filter_group<DT, NS>(c, z, cur));
      cur = nxt;
    }
    for (uint64_t j = whole; j < p.n_samples; ++j) out[j] = filter_word<DT, NS>(c, z, in[j]);
#pragma unroll
    for (int k = 0; k < 2 * NS; ++k) st[k] = z[k];                   // (the words of sections that do not exist stay as they are)
  }
}

template <int DT, int NS>
void launch_one(unsigned grid, hipStream_t hs, const Params& p) {
  hipLaunchKernelGGL((iir_kernel<DT, NS>), dim3(grid), dim3(LANES), 0, hs, p);
}

template <int DT>
int launch_dtype(int n_sections, unsigned grid, hipStream_t hs, const Params& p) {
  switch (n_sections) {
    case 1: launch_one<DT, 1>(grid, hs, p); break;
    case 2: launch_one<DT, 2>(grid, hs, p); break;
    case 3: launch_one<DT, 3>(grid, hs, p); break;
    case 4: launch_one<DT, 4>(grid, hs, p); break;
    case 5: launch_one<DT, 5>(grid, hs, p); break;
    case 6: launch_one<DT, 6>(grid, hs, p); break;
    case 7: launch_one<DT, 7>(grid, hs, p); break;
    case 8: launch_one<DT, 8>(grid, hs, p); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

}  // namespace

int launch_filter(int dtype, int n_sections, unsigned grid, void* stream, const Params& p) {
  hipStream_t hs = (hipStream_t)stream;
  switch (dtype) {
    case DT_F32: return launch_dtype<DT_F32>(n_sections, grid, hs, p);
    case DT_I32: return launch_dtype<DT_I32>(n_sections, grid, hs, p);
    default: return (int)hipErrorInvalidValue;
  }
}

}  // namespace uc_iir_dev
