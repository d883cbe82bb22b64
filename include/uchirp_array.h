/* uchirp_array.h -- C-ABI of libuchirp_array.so: the array combiner of the chirp modem (delay-and-sum beams).
 *
 * uc_scene_render (uchirp_scene.h) gives every microphone of an array the same transmission at its own fractional lead,
 * plus echoes, interferers and independent noise.  The combiner is the stage between that buffer (or a recorded one)
 * and the receivers of uchirp.h: every BEAM is a weighted sum of microphones, each shifted in time by its own fractional
 * delay, so that the wanted sound adds in phase while noise and sounds from elsewhere do not.
 *
 * The library stands alone: it needs no symbol of libuchirp.so, libuchirp_link.so or libuchirp_scene.so.  There is no
 * CPU path: uc_array_create fails without a GPU.  uc_array_tap_coefficients is pure host arithmetic and works anywhere.
 *
 * DEFINITION
 *
 * Input.  n_mics rows in device memory, UC_ARRAY_DTYPE_F32 (float) or UC_ARRAY_DTYPE_I32 (DFSDM words, each cast with
 * (float) as the receivers do).  Row m starts at in_dev + m * in_stride (elements) and holds the absolute samples
 * [in_first, in_first + n_in).  A sample outside that range reads as +0.0f.  x_k[j] below is sample j of the row of
 * tap k's microphone, after the cast.
 *
 * Tap.  { delay_samples, weight, mic }: this microphone hears the wanted sound delay_samples LATER than the beam's time
 * axis.  For a scene path of lead L_m and a wanted beam lead L_0 the delay is L_m - L_0.
 *
 * Beam.  { first_tap, n_taps }: taps[first_tap] .. taps[first_tap + n_taps - 1], in that order; n_taps is
 * 1 .. UC_ARRAY_MAX_TAPS.  Tap ranges of different beams may overlap.
 *
 * Coefficients (uc_array_tap_coefficients; evaluated on the host in double, once per tap and call: the device never
 * evaluates a sinc).  For D = delay_samples let I = floor(D) and f = D - I (should the subtraction round to 1.0, as for a
 * tiny negative D, I + 1 and f = 0 are taken).  shift = I - 7, and
 *   f == 0:    c[7] = weight, every other c[t] = 0
 *   otherwise  c[t] = (float)(weight * sinc(u) * I0(8 * sqrt(1 - (u / 8)^2)) / I0(8)),  u = t - 7 - f,  t = 0 .. 15
 * with sinc(u) = sin(pi u) / (pi u) and I0 the modified Bessel function of order 0: a 16-tap Kaiser (beta = 8) windowed
 * sinc.
 *
 * Output.  Beam b, absolute sample j in [out_first, out_first + n_out), is a float stored at
 * out_dev + b * out_stride + (j - out_first):
 *   a_k = c_k[0] * x_k[j + shift_k];  a_k = fmaf(c_k[t], x_k[j + shift_k + t], a_k)  for t = 1 .. 15
 *   y = a_0;  y = y + a_k  for k = 1 .. n_taps - 1      (each addition rounded once: no fused multiply-add)
 * A value depends on the inputs and the taps only, never on the grid, the tile, or how the output range is cut into
 * calls.  One tap with weight 1 and an integer delay is a copy of the microphone shifted by that delay, equal as floats,
 * for FINITE inputs: the chain still multiplies the 15 neighbouring samples by 0.0f, so an infinity or a NaN within
 * -7 .. +8 samples of a sample makes that output NaN (as it does for every fractional delay).
 *
 * Non-finite samples.  One float sample x_m[q] that is NaN, +Inf or -Inf (integer words hold none):
 *   MUST      output j of a beam is not finite wherever one of its taps k of microphone m has q under its sixteen
 *             coefficients, j + shift_k <= q <= j + shift_k + 15 (shift_k from uc_array_tap_coefficients) -- also where
 *             c_k[t] is zero, as fifteen are for an integer delay: 0 * NaN is NaN.
 *   MAY       nothing: every chain is evaluated as it is written.
 *   MUST NOT  every other output of the beam, the beams without a tap of microphone m, and every word of out_dev between
 *             the rows: bit for bit what the same call writes with a finite sample there.  A sample whose supports all lie
 *             outside [out_first, out_first + n_out) touches nothing.
 *
 * OUT OF SCOPE: per-microphone clock offsets (an array shares one clock here; libuchirp_retime.so, uchirp_retime.h, puts
 * microphones with clocks of their own onto one first); estimating the delays (that is libuchirp_align.so, uchirp_align.h);
 * adaptive weights; output formats other than float; capture into a graph.
 */
#ifndef UCHIRP_ARRAY_H
#define UCHIRP_ARRAY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UC_ARRAY_ABI_VERSION 1

#define UC_ARRAY_DTYPE_I32 0 /* DFSDM words */
#define UC_ARRAY_DTYPE_F32 1

#define UC_ARRAY_MAX_TAPS 32  /* per beam */
#define UC_ARRAY_COEFS 16     /* coefficients of one tap */

typedef struct uc_array uc_array;

/* one microphone of one beam (16 bytes) */
typedef struct uc_array_tap {
  double delay_samples; /* finite, |delay_samples| <= 2^30 */
  float weight;         /* finite */
  uint32_t mic;         /* row of the input (< n_mics) */
} uc_array_tap;

/* one beam (8 bytes): taps[first_tap .. first_tap + n_taps - 1] */
typedef struct uc_array_beam {
  uint32_t first_tap;
  uint32_t n_taps; /* 1 .. UC_ARRAY_MAX_TAPS */
} uc_array_beam;

int uc_array_abi_version(void);
/* text of the calling thread's last error ("" if none) */
const char* uc_array_last_error(void);
/* -ENODEV ("no CPU path") when no GPU is visible */
int uc_array_create(int device, uc_array** out);
/* Waits for every call of the object still in flight, on whatever streams they were given (each call is ordered behind the
 * call two before it, so the events of the last two cover all), then frees it.  NULL is allowed. */
void uc_array_destroy(uc_array* array);

/* The coefficients of the definition; needs no GPU.  -EINVAL: a NULL pointer, delay_samples or weight not finite,
 * |delay_samples| > 2^30. */
int uc_array_tap_coefficients(double delay_samples, float weight, int64_t* shift, float coef[UC_ARRAY_COEFS]);

/* Writes samples [out_first, out_first + n_out) of n_beams beams.  taps (n_taps) and beams (n_beams) are HOST arrays:
 * they are copied, with the records derived from them, into one of two pinned staging buffers of the object, used in
 * turn, before the call returns (the caller may reuse them at once), and from there to the device on hip_stream.
 * in_dev and out_dev are device memory of the object's device; strides are in elements, 0 means the count (n_in, n_out).
 * Asynchronous on hip_stream (a hipStream_t, or NULL); the caller's current HIP device is restored.  Every argument is
 * checked and every buffer is sized before anything is enqueued: a refused call (negative errno) has enqueued nothing and
 * leaves the object usable.  -EINVAL: a tap's mic >= n_mics; a beam beyond n_taps, or with 0 or more than
 * UC_ARRAY_MAX_TAPS taps; a delay or weight that is not finite, or |delay| > 2^30; a stride smaller than its count; an
 * unknown dtype; a zero count; a NULL array; in_dev or out_dev not device memory of the object's device; out_dev
 * overlapping in_dev.  One thread at a time per object; not capturable into a graph. */
int uc_array_combine(uc_array* array, const void* in_dev, int in_dtype, size_t n_mics, uint64_t in_first, size_t n_in,
                     size_t in_stride, const uc_array_tap* taps, size_t n_taps, const uc_array_beam* beams, size_t n_beams,
                     float* out_dev, uint64_t out_first, size_t n_out, size_t out_stride, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
