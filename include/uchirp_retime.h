/* uchirp_retime.h -- C-ABI of libuchirp_retime.so: the retimer of the chirp modem (microphones with their own clocks).
 *
 * uc_array_combine (uchirp_array.h) shifts every microphone by a CONSTANT fractional delay: an array there shares one
 * clock.  Independent microphones (USB capsules, separate boards) differ by tens of ppm, and over a message that is many
 * carrier periods.  The retimer is the stage in front of the combiner and the correlators: output row r is input row mic_r
 * read along a LINE p(j) = j + delay_r + slope_r * j, a fractional delay that varies with time, applied in one pass.
 *
 * The library stands alone: it needs no symbol of the other six libraries.  There is no CPU path: uc_retime_create fails
 * without a GPU.  uc_retime_fixed and uc_retime_table are pure host arithmetic and work anywhere.
 *
 * DEFINITION
 *
 * Input.  n_mics rows in device memory, UC_RETIME_DTYPE_F32 (float) or UC_RETIME_DTYPE_I32 (DFSDM words, each cast with
 * (float) as the receivers do).  Row m starts at in_dev + m * in_stride (elements) and holds the absolute samples
 * [in_first, in_first + n_in).  A sample outside that range reads as +0.0f.  x[i] below is sample i of the row of the
 * line's microphone, after the cast.
 *
 * Line.  { delay_samples, slope, mic, reserved = 0 }: output sample j (an absolute sample number) reads the input at
 * position j + delay_samples + slope * j.  delay_samples has the sign of uc_array_tap.delay_samples: this microphone hears
 * the sound that much LATER than the output's time axis.
 *
 * Fixed point (uc_retime_fixed; on the host, once per line and call).  lead_fx = llrint(delay_samples * 2^32) and
 * drift_fx = llrint(slope * 2^32); |delay_samples| <= 2^30 and |slope| <= 2^-9 (1953 ppm), so |drift_fx| <= 2^23.  The device
 * works from these two integers only, in exact 64-bit integer arithmetic.  For absolute output sample j < 2^38:
 *   off  = lead_fx + j * drift_fx            (no overflow: 2^38 * 2^23 + 2^62 < 2^63)
 *   I    = j + (off >> 32)                   (arithmetic shift)
 *   frac = off & 0xffffffff;  q = frac >> 24 (0 .. 255);  mu = (float)(frac & 0xffffff) * 2^-24   (exact)
 *
 * Table (uc_retime_table; on the host, once per object).  T[257][16] floats.  Row q < 256 holds the 16-tap Kaiser
 * (beta = 8) windowed sinc of uchirp_array.h at the fraction f = q / 256 and weight 1:
 *   f == 0:    T[0][7] = 1, every other T[0][t] = 0
 *   otherwise  T[q][t] = (float)(sinc(u) * I0(8 * sqrt(1 - (u / 8)^2)) / I0(8)),  u = t - 7 - f,  t = 0 .. 15
 * evaluated in double and rounded to float: the values uc_array_tap_coefficients gives.  Row 256 is the unit at t = 8 (the
 * fraction 1 is the next sample).  D[q][t] = T[q + 1][t] - T[q][t], the float subtraction of the float entries.
 *
 * Output.  Row r, absolute sample j in [out_first, out_first + n_out), is a float stored at
 * out_dev + r * out_stride + (j - out_first):
 *   c[t] = fmaf(mu, D[q][t], T[q][t])                                     t = 0 .. 15
 *   y = c[0] * x[I - 7];  y = fmaf(c[t], x[I - 7 + t], y)  for t = 1 .. 15
 * A value depends on the inputs and the line only, never on the grid, the tile, the other lines, or how the output range is
 * cut into calls.  slope = 0 and an integer delay give a copy of the microphone shifted by that delay, equal as floats,
 * for FINITE inputs (the chain still multiplies the 15 neighbouring samples by 0.0f).  slope = 0 and a delay of k + q / 256
 * give what uc_array_combine gives for one tap of weight 1 at that delay, bit for bit.
 *
 * Non-finite samples.  One float sample x[i] of microphone m that is NaN, +Inf or -Inf (integer words hold none):
 *   MUST      output j of a line of microphone m is not finite wherever I - 7 <= i <= I + 8, with I the integer of the
 *             fixed-point step above -- all sixteen coefficients, also where c[t] is zero, as fifteen are on a whole
 *             sample (q = 0 and mu = 0): 0 * NaN is NaN.
 *   MAY       nothing: the chain is evaluated as it is written.
 *   MUST NOT  every other output of the line, the lines of other microphones, and every word of out_dev between the
 *             rows: bit for bit what the same call writes with a finite sample there.  A sample whose supports all lie
 *             outside [out_first, out_first + n_out) touches nothing.
 *
 * OUT OF SCOPE: ratios far from 1 (rate conversion between 44.1, 48 and 96 kHz needs other filters); estimating the line on
 * the GPU (uchirp/retime.py fits it on the host from the windows of libuchirp_align.so or libuchirp_xcorr.so); output formats
 * other than float; capture into a graph.
 */
#ifndef UCHIRP_RETIME_H
#define UCHIRP_RETIME_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UC_RETIME_ABI_VERSION 1

#define UC_RETIME_DTYPE_I32 0 /* DFSDM words */
#define UC_RETIME_DTYPE_F32 1

#define UC_RETIME_COEFS 16      /* coefficients of one output sample */
#define UC_RETIME_TABLE_ROWS 257 /* fractions 0, 1/256 .. 255/256, 1 */

typedef struct uc_retime uc_retime;

/* one output row (24 bytes) */
typedef struct uc_retime_line {
  double delay_samples; /* finite, |delay_samples| <= 2^30 */
  double slope;         /* finite, |slope| <= 2^-9 */
  uint32_t mic;         /* row of the input (< n_mics) */
  uint32_t reserved;    /* 0 */
} uc_retime_line;

int uc_retime_abi_version(void);
/* text of the calling thread's last error ("" if none) */
const char* uc_retime_last_error(void);
/* -ENODEV ("no CPU path") when no GPU is visible */
int uc_retime_create(int device, uc_retime** out);
/* Waits for every call of the object still in flight, on whatever streams they were given (each call is ordered behind the
 * call two before it, so the events of the last two cover all), then frees it.  NULL is allowed. */
void uc_retime_destroy(uc_retime* retime);

/* The two integers of the definition; needs no GPU.  -EINVAL: a NULL pointer, delay_samples or slope not finite,
 * |delay_samples| > 2^30, |slope| > 2^-9. */
int uc_retime_fixed(double delay_samples, double slope, int64_t* lead_fx, int64_t* drift_fx);

/* The table of the definition, T[q][t] at table[16 * q + t]; needs no GPU.  -EINVAL: a NULL pointer. */
int uc_retime_table(float table[UC_RETIME_TABLE_ROWS * UC_RETIME_COEFS]);

/* Writes samples [out_first, out_first + n_out) of n_lines rows.  lines (n_lines) is a HOST array: it is copied, as the
 * records derived from it, into one of two pinned staging buffers of the object, used in turn, before the call returns (the
 * caller may reuse it at once), and from there to the device on hip_stream.  in_dev and out_dev are device memory of the
 * object's device; strides are in elements, 0 means the count (n_in, n_out).  Asynchronous on hip_stream (a hipStream_t, or
 * NULL); the caller's current HIP device is restored.  Every argument is checked and every buffer is sized before anything
 * is enqueued: a refused call (negative errno) has enqueued nothing and leaves the object usable.  -EINVAL: a line's
 * mic >= n_mics; a line that uc_retime_fixed refuses; reserved != 0; out_first + n_out > 2^38; a stride smaller than its
 * count; an unknown dtype; a zero count; a NULL array; in_dev or out_dev not device memory of the object's device; out_dev
 * overlapping in_dev.  One thread at a time per object; not capturable into a graph. */
int uc_retime_rows(uc_retime* retime, const void* in_dev, int in_dtype, size_t n_mics, uint64_t in_first, size_t n_in,
                   size_t in_stride, const uc_retime_line* lines, size_t n_lines, float* out_dev, uint64_t out_first,
                   size_t n_out, size_t out_stride, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
