// uc_dfsdm_kernel.hip -- the DFSDM filter's kernel (gfx950): every row of packed PDM words becomes the words of the
// peripheral's filter in any of its configurations: FastSinc or Sinc1..5, ratio 1..1024, integrator 1..256, right shift and
// offset.  include/uchirp_dfsdm.h states the definition; uchirp/dfsdm.py holds it in numpy (`model`); uc_dfsdm.hpp holds the
// arithmetic itself, shared with uc_dfsdm_filter_row.
//
// The integrators are a recurrence along the row, so the parallel axis is the rows: a lane is one row, a wave 64 rows, a
// workgroup ONE wave, so that 1024 workgroups (65 536 bit streams) are one wave on each of the chip's 1024 SIMDs.  A lane
// reads its row's state once, walks the row and writes the state once.  One long recording runs on one lane.
//
// Two paths, the same bits:
//   the word path   R a multiple of 32.  Over one word the integrators advance by a constant matrix plus a vector that
//                   depends on the word's four bytes: four lookups in LDS tables [byte position][byte value] (each byte's
//                   contribution already carried to the end of the word), one matrix application (uc_dfsdm.hpp:
//                   advance_word), and at every R-th bit the combs, at every I-th value the shift and the clip.
//   the bit path    every other ratio: the definition's loop over the word's bits (uc_dfsdm.hpp: word_by_bits); a word
//                   gives up to 32 outputs.
//
// The lookups are indexed by data bytes.  Every row of a call stands at the same bit, so the ORDER in which a lane takes
// its word's four bytes is free: in step i lane l takes byte (i + (l >> 2)) & 3, and the tables lie entry 4 v + b, so that
// the 16 lanes one LDS cycle of a 16-byte read serves -- four runs of four lanes with four different l >> 2 & 3 -- look at
// four byte positions that own four banks each; only the four lanes that share a position can still meet.
//
// Memory as in the microphone model's kernel (profiles/r18_mic.txt is why): where pointers and strides put every row on 16
// bytes the wave moves TILES of 64 rows x 16 words through LDS, four lanes to one row's 64 contiguous bytes, the next input
// tile's loads in flight while this one is filtered.  Every row of a call gives its outputs at the same bits, so the
// output tile fills in step across the lanes and leaves when it holds 16 words.  What is left behind the last whole input
// tile -- and everything where a pointer or stride does not put the rows on 16 bytes -- goes direct, as dwords.
//
// All arithmetic is int32 with wrap-around (unsigned in the code), so the words depend on the row's bits, its state and
// words_before only, never on the path or the grid: row blocks are dealt blockIdx.x, + gridDim.x, ...
#include <hip/hip_runtime.h>

#include "uc_dfsdm.hpp"

namespace uc_dfsdm_dev {
namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

constexpr int TILE = 16;                 // words of a row in one staged tile: 64 bytes, four 16-byte pieces
constexpr int PITCH = 5;                 // 16-byte units between two rows of a tile in LDS: four pieces and one of padding
constexpr int SWEEPS = LANES / 16;       // a load instruction covers 16 rows (4 lanes a row): 4 of them cover the tile

// where a row's outputs go: into the lane's row of the output tile (`tiled`, every lane goes along) or straight to memory
struct Sink {
  uint32_t* tile;          // the lane's 16 words of the output tile
  u4* tile_all;            // the whole tile
  int32_t* row;            // the lane's output row
  int32_t* dst[SWEEPS];    // of the tile's moves: where piece `piece` of row sub + 16 k starts
  bool there[SWEEPS];
  uint32_t sub, piece;
  uint64_t n_out;          // of the call, per row: what the host's plan and the phase both say
  uint64_t done;           // outputs given so far (uniform)
  uint32_t fill;           // of them, in the tile (uniform)
  bool tiled, live;

  __device__ __forceinline__ void operator()(int32_t word) {
    if (tiled) {
      tile[fill] = (uint32_t)word;
      if (++fill == TILE) flush_tile();
    } else if (live && done < n_out) {
      row[done] = word;
    }
    ++done;
  }
  // a full tile: 16 rows a store instruction, 64 contiguous bytes a row
  __device__ __forceinline__ void flush_tile() {
    __syncthreads();
    const uint64_t at = done + 1 - TILE;                             // (done counts this word behind the call)
#pragma unroll
    for (int k = 0; k < SWEEPS; ++k)
      if (there[k]) *reinterpret_cast<u4*>(dst[k] + at) = tile_all[(sub + 16 * k) * PITCH + piece];
    __syncthreads();
    fill = 0;
  }
  // what the tile holds behind the row's last output
  __device__ __forceinline__ void flush_rest() {
    if (tiled && live)
      for (uint32_t j = 0; j < fill; ++j) row[done - fill + j] = (int32_t)tile[j];
  }
};

template <int ORDER>
__device__ __forceinline__ void word_by_table(State<ORDER>& s, uint32_t w, Phase& ph, const Params& p, const u4* tab4, const uint32_t* tab1,
                                              uint32_t rot, Sink& sink) {
  constexpr int N = State<ORDER>::N;
  uint32_t add[N];
#pragma unroll
  for (int k = 0; k < N; ++k) add[k] = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t b = (i + rot) & 3u;
    const uint32_t e = (((w >> (8u * b)) & 255u) << 2) | b;         // entry 4 v + b
    const u4 q = tab4[e];
    add[0] += q.x;
    if (N > 1) add[N > 1 ? 1 : 0] += q.y;
    if (N > 2) add[N > 2 ? 2 : 0] += q.z;
    if (N > 3) add[N > 3 ? 3 : 0] += q.w;
    if (N > 4) add[N > 4 ? 4 : 0] += tab1[e];
  }
  advance_word(s.integ, add);
  ph.r += 32;
  if (ph.r == p.ratio) {
    ph.r = 0;
    decimate(s);
    if (++ph.i == p.integ) {
      ph.i = 0;
      sink(output_word(s, p.shift, p.offset));
    }
  }
}

template <int ORDER, bool WORD>
__global__ __launch_bounds__(LANES) void dfsdm_kernel(const Params p) {
  constexpr int N = State<ORDER>::N;
  __shared__ u4 tile_in[LANES * PITCH], tile_out[LANES * PITCH];
  __shared__ u4 tab4[WORD ? TABLE_ENTRIES : 1];
  __shared__ uint32_t tab1[WORD && N > 4 ? TABLE_ENTRIES : 1];
  const uint32_t lane = threadIdx.x;
  const uint32_t piece = lane & 3u, sub = lane >> 2;                // of the tile's moves: lane = (row sub + 16 k, piece)
  const bool in_vec = p.in_vec != 0;
  if (WORD) {
    // entry 256 b + v of the object's tables -> entry 4 v + b here
    for (uint32_t e = lane; e < (uint32_t)TABLE_ENTRIES; e += LANES) {
      const uint32_t to = ((e & 255u) << 2) | (e >> 8);
      tab4[to] = reinterpret_cast<const u4*>(p.table)[e];
      if (N > 4) tab1[to] = (uint32_t)p.table[4 * TABLE_ENTRIES + e];
    }
    __syncthreads();
  }
  const uint64_t tiles = in_vec ? p.n_words / TILE : 0;
  for (uint32_t rb = blockIdx.x; rb < p.row_blocks; rb += gridDim.x) {
    const uint64_t row0 = (uint64_t)rb * LANES;
    const uint64_t r = row0 + lane;
    const bool live = r < p.n_rows;                                 // (a lane without a row goes along with zeros; it touches no memory)
    const uint32_t* const in = p.in + (live ? r : 0) * p.in_stride;
    int32_t* const st = p.state + (live ? r : 0) * STATE_WORDS;
    State<ORDER> s;
    {
      int32_t zero[STATE_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      load_state(s, zero);
    }
    if (live) load_state(s, st);                                    // (dwords: once per row, and any alignment will do)
    Phase ph = {p.phase_r, p.phase_i};
    Sink sink;
    sink.tile = reinterpret_cast<uint32_t*>(&tile_out[lane * PITCH]);
    sink.tile_all = tile_out;
    sink.row = p.out + (live ? r : 0) * p.out_stride;
    sink.sub = sub;
    sink.piece = piece;
    sink.n_out = p.n_out;
    sink.done = 0;
    sink.fill = 0;
    sink.tiled = p.out_vec != 0;
    sink.live = live;
    const uint32_t* src[SWEEPS];
    bool there[SWEEPS];
#pragma unroll
    for (int k = 0; k < SWEEPS; ++k) {
      const uint64_t row = row0 + sub + 16 * k;
      there[k] = row < p.n_rows;
      sink.there[k] = there[k];
      src[k] = p.in + (there[k] ? row : 0) * p.in_stride + piece * 4;
      sink.dst[k] = p.out + (there[k] ? row : 0) * p.out_stride + piece * 4;
    }

    // ---- whole input tiles through LDS
    if (tiles) {
      u4 nxt[SWEEPS];
#pragma unroll
      for (int k = 0; k < SWEEPS; ++k) {
        nxt[k] = u4{0, 0, 0, 0};
        if (there[k]) nxt[k] = *reinterpret_cast<const u4*>(src[k]);
      }
      for (uint64_t t = 0; t < tiles; ++t) {
        __syncthreads();                                            // (one wave: the last tile's words have been read)
#pragma unroll
        for (int k = 0; k < SWEEPS; ++k) tile_in[(sub + 16 * k) * PITCH + piece] = nxt[k];
        __syncthreads();
        if (t + 1 < tiles) {
#pragma unroll
          for (int k = 0; k < SWEEPS; ++k)
            if (there[k]) nxt[k] = *reinterpret_cast<const u4*>(src[k] + (t + 1) * TILE);
        }
#pragma unroll 1
        for (int g = 0; g < TILE / 4; ++g) {
          const u4 x = tile_in[lane * PITCH + g];                   // (16 bytes: rows 20 words apart fall on 64 banks)
          const uint32_t w4[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (WORD)
              word_by_table<ORDER>(s, w4[j], ph, p, tab4, tab1, lane >> 2, sink);
            else
              word_by_bits<ORDER>(s, w4[j], ph, p.ratio, p.integ, p.shift, p.offset, sink);
          }
        }
      }
    }

    // ---- the rest of the row (all of it where the input's rows are not on 16 bytes), direct
    for (uint64_t j = tiles * TILE; j < p.n_words; ++j) {
      const uint32_t w = live ? in[j] : 0u;
      if (WORD)
        word_by_table<ORDER>(s, w, ph, p, tab4, tab1, lane >> 2, sink);
      else
        word_by_bits<ORDER>(s, w, ph, p.ratio, p.integ, p.shift, p.offset, sink);
    }
    sink.flush_rest();
    if (live) store_state(s, st);
    __syncthreads();                                                // (the next row block writes the output tile again)
  }
}

template <int ORDER>
hipError_t launch_order(bool word_path, unsigned grid, hipStream_t hs, const Params& p) {
  if (word_path)
    hipLaunchKernelGGL((dfsdm_kernel<ORDER, true>), dim3(grid), dim3(LANES), 0, hs, p);
  else
    hipLaunchKernelGGL((dfsdm_kernel<ORDER, false>), dim3(grid), dim3(LANES), 0, hs, p);
  return hipGetLastError();
}

}  // namespace

int launch_filter(int order, bool word_path, unsigned grid, void* stream, const Params& p) {
  hipStream_t hs = (hipStream_t)stream;
  switch (order) {
    case 0: return (int)launch_order<0>(word_path, grid, hs, p);
    case 1: return (int)launch_order<1>(word_path, grid, hs, p);
    case 2: return (int)launch_order<2>(word_path, grid, hs, p);
    case 3: return (int)launch_order<3>(word_path, grid, hs, p);
    case 4: return (int)launch_order<4>(word_path, grid, hs, p);
    case 5: return (int)launch_order<5>(word_path, grid, hs, p);
    default: return (int)hipErrorInvalidValue;
  }
}

}  // namespace uc_dfsdm_dev
