/* uchirp_rate.h -- C-ABI of libuchirp_rate.so: the rate converter of the chirp modem (sound-card rates to the receivers'
 * 78 125 Hz).
 *
 * Every receiver of this project reads samples at 78 125 Hz.  A sound card delivers 44.1, 48 or 96 kHz, and the transmitter
 * the project pins itself to is a 44.1 kHz WAV.  uc_rate_convert is the stage in front of everything else: n_rows rows at
 * one rate in, the same rows at up / down times that rate out, through one polyphase Kaiser-windowed sinc, in one pass.
 *
 * The library stands alone: it needs no symbol of the other eight libraries.  There is no CPU path: uc_rate_create fails
 * without a GPU.  uc_rate_plan, uc_rate_table, uc_rate_step, uc_rate_span and uc_rate_count are pure host arithmetic and
 * work anywhere.
 *
 * DEFINITION  (uchirp/rate.py holds it in float64: `model`; on whole rows from sample 0 it is uchirp/resample.py's
 * resample(x, up, down, half, beta))
 *
 * Ratio.  up / down, reduced by their greatest common divisor by the library.  After the reduction 1 <= up, down <= 4096
 * and up != down (the ratio 1 is refused).  half is in 4 .. 32, beta is finite and in 0 .. 100.  q = max(up, down),
 * N_h = 2 half q + 1, centre c = half q.
 *
 * Prototype, evaluated in double, i = 0 .. N_h - 1:
 *   g[i] = sinc((i - c) / q) * I0(beta * sqrt(1 - ((i - c) / c)^2)) / I0(beta)        sinc(0) = 1, sinc(u) = sin(pi u) / (pi u)
 *   h[i] = g[i] * up / sum g                                                          (the sum in the order of i)
 *
 * Taps.  T = (2 half q) div up + 1 input samples under one output.  T <= 128 and up * T <= 2^19, otherwise -EINVAL.
 * 44.1 kHz -> 78 125 Hz is 3125 / 1764 with T = 49 (153 125 table floats), 48 kHz is 625 / 384 with T = 49, 96 kHz is
 * 625 / 768 with T = 59.
 *
 * Table (uc_rate_table; on the host, once per object).  C[p][j] = (float) h[p + j up] where p + j up < N_h, else 0;
 * p = 0 .. up - 1, j = 0 .. T - 1; C[p][j] lies at table[p * T + j].
 *
 * Position (uc_rate_step), in exact 64-bit integers, for absolute output sample m < 2^38:
 *   pos = m down + c,   k = pos div up,   p = pos mod up
 * Output sample 0 lies on input sample 0 (zero delay).
 *
 * Input.  n_rows rows in device memory, UC_RATE_DTYPE_I16 (WAV PCM) or UC_RATE_DTYPE_F32; every sample is cast with
 * (float).  Row r starts at in_dev + r * in_stride (elements) and holds the absolute samples [in_first, in_first + n_in).
 * Every other sample reads as +0.0f, the samples before 0 among them.  x[i] below is sample i of the row, after the cast.
 *
 * Output.  Row r, absolute sample m in [out_first, out_first + n_out), is a float stored at
 * out_dev + r * out_stride + (m - out_first):
 *   y = C[p][T - 1] * x[k - T + 1];   y = fmaf(C[p][j], x[k - j], y)  for j = T - 2 .. 0
 * the oldest input first, one accumulator.  A value depends on the row's samples and m only, never on the grid, the tile,
 * the other rows, or how the output range is cut into calls.  (The order ascends in the input index: a kernel that feeds a
 * banded coefficient tile to the f32 matrix instruction, itself an fmaf chain, meets it too, for finite inputs.)
 *
 * Non-finite samples.  One float sample x[q] of row r that is NaN, +Inf or -Inf (int16 samples hold none):
 *   MUST      output m of row r is not finite wherever its chain has a term with x[q]: k - T + 1 <= q <= k, with k the
 *             newest input of m (uc_rate_step) -- all T taps, also where C[p][j] is zero (the taps behind the prototype's
 *             end, the zeros of the sinc at integer phases): 0 * NaN is NaN.
 *   MAY       nothing: the chain is evaluated as it is written, one accumulator per output and row.
 *   MUST NOT  every other output of the row, every other row (the fifteen that share its block and its packed
 *             multiply-adds among them), and every word of out_dev between the rows: bit for bit what the same call writes
 *             with a finite sample there.
 *
 * OUT OF SCOPE: ratios that change during a call (the retimer's job, uchirp_retime.h, behind this stage); output formats
 * other than float; a selection of rows; capture into a graph; filters other than the Kaiser family.
 */
#ifndef UCHIRP_RATE_H
#define UCHIRP_RATE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UC_RATE_ABI_VERSION 1

#define UC_RATE_DTYPE_I16 0 /* WAV PCM */
#define UC_RATE_DTYPE_F32 1

#define UC_RATE_RATIO_MAX 4096      /* up and down after the reduction */
#define UC_RATE_HALF_MIN 4
#define UC_RATE_HALF_MAX 32
#define UC_RATE_TAPS_MAX 128
#define UC_RATE_TABLE_MAX (1u << 19) /* up * taps */

typedef struct uc_rate uc_rate;

/* what uc_rate_plan makes of a ratio (24 bytes) */
typedef struct uc_rate_info {
  uint32_t up;        /* reduced */
  uint32_t down;      /* reduced */
  uint32_t half;
  uint32_t taps;      /* T */
  uint32_t centre;    /* c = half * max(up, down) */
  uint32_t table_len; /* up * T floats */
} uc_rate_info;

int uc_rate_abi_version(void);
/* text of the calling thread's last error ("" if none) */
const char* uc_rate_last_error(void);

/* The plan of the definition; needs no GPU.  -EINVAL: info is NULL; up or down is 0; after the reduction up == down, up or
 * down > 4096, T > 128 or up * T > 2^19; half not in 4 .. 32; beta not finite or not in 0 .. 100. */
int uc_rate_plan(uint32_t up, uint32_t down, uint32_t half, double beta, uc_rate_info* info);

/* The table of the definition, C[p][j] at table[p * taps + j]; needs no GPU.  -EINVAL: a NULL pointer, an info that
 * uc_rate_plan did not make, a beta it refuses, len != info->table_len. */
int uc_rate_table(const uc_rate_info* info, double beta, float* table, size_t len);

/* k and p of output sample m; needs no GPU.  -EINVAL: a NULL pointer, an info that uc_rate_plan did not make, m >= 2^38. */
int uc_rate_step(const uc_rate_info* info, uint64_t m, int64_t* k, uint32_t* phase);

/* The input samples that the outputs [out_first, out_first + n_out) read: [*in_lo, *in_hi), in_lo = k(out_first) - T + 1
 * (negative near sample 0: those read as 0), in_hi = k(out_first + n_out - 1) + 1; needs no GPU.  A live caller learns
 * from it what an output block of 2048 samples needs.  -EINVAL: a NULL pointer, an info that uc_rate_plan did not make,
 * n_out == 0, out_first + n_out > 2^38. */
int uc_rate_span(const uc_rate_info* info, uint64_t out_first, size_t n_out, int64_t* in_lo, int64_t* in_hi);

/* ceil(n_in * up / down): the outputs that n_in input samples from sample 0 stand for (resample's count); needs no GPU.
 * -EINVAL: info is NULL or not one that uc_rate_plan made, n_in > 2^40. */
int64_t uc_rate_count(const uc_rate_info* info, uint64_t n_in);

/* An object for one ratio on one device; the table is computed and uploaded once.  -EINVAL as uc_rate_plan; -ENODEV ("no
 * CPU path") when no GPU is visible. */
int uc_rate_create(int device, uint32_t up, uint32_t down, uint32_t half, double beta, uc_rate** out);
/* Waits for the device, and with it for every call of the object on whatever stream it was given (a call that stages
 * nothing leaves no event to wait for), then frees it.  NULL is allowed. */
void uc_rate_destroy(uc_rate* rate);

/* Writes samples [out_first, out_first + n_out) of n_rows rows.  in_dev and out_dev are device memory of the object's
 * device; strides are in elements, 0 means the count (n_in, n_out).  Asynchronous on hip_stream (a hipStream_t, or NULL);
 * the caller's current HIP device is restored.  The call reads no host array: all it needs travels as kernel arguments, so
 * nothing is staged and calls in a row do not wait for each other on the host.  Every argument is checked before anything
 * is enqueued: a refused call (negative errno) has enqueued nothing and leaves the object usable.  -EINVAL:
 * out_first + n_out > 2^38; a stride smaller than its count; an unknown dtype; a zero count; a NULL pointer; in_dev or
 * out_dev not device memory of the object's device; out_dev overlapping in_dev.  One thread at a time per object; not
 * capturable into a graph. */
int uc_rate_convert(uc_rate* rate, const void* in_dev, int in_dtype, size_t n_rows, uint64_t in_first, size_t n_in,
                    size_t in_stride, float* out_dev, uint64_t out_first, size_t n_out, size_t out_stride, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
