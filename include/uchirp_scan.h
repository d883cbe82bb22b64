/* uchirp_scan.h -- C-ABI of libuchirp_scan.so: the beam scanner of the chirp modem (the power of every steered beam per
 * window).
 *
 * The array combiner (uchirp_array.h) steers a beam once it is told every microphone's delay; the estimators (uchirp_align.h,
 * uchirp_xcorr.h, uchirp_track.h, uchirp_wcorr.h) get those delays pair by pair, and at low SNR a pair lands whole carrier
 * cycles off.  The array's geometry allows only a small family of delay vectors.  The scanner forms the delay-and-sum beam
 * of EVERY candidate vector, measures its power per window, and names the strongest: the microphones are read once and one
 * number per (array, window, beam) is written.
 *
 * The library stands alone: it needs no symbol of the other libraries.  There is no CPU path behind uc_scan_power:
 * uc_scan_create fails without a GPU.  uc_scan_quantise, uc_scan_table and uc_scan_power_row are host functions and work
 * anywhere.
 *
 * DEFINITION
 *
 * Input.  n_rows rows in device memory, UC_SCAN_DTYPE_F32 (float) or UC_SCAN_DTYPE_I32 (DFSDM words, each cast with (float)
 * as the array combiner does).  Row r starts at in_dev + r * in_stride (elements) and holds the absolute samples
 * [in_first, in_first + n_in).  A sample outside that range reads as +0.0f.
 *
 * Arrays.  n_arrays arrays of array_rows rows each; array a owns rows a * array_rows .. (a + 1) * array_rows - 1.  All
 * arrays share one steering set.
 *
 * Steering set (uc_scan_set_beams; held by the object).  n_taps microphones, 1 .. UC_SCAN_MAX_TAPS; mics[k] < array_rows
 * is tap k's row within an array; weights[k] a finite float; n_beams x n_taps delays (doubles, finite, |d| <= 2^20,
 * 1 <= n_beams <= 2^20): delays[b * delay_stride + k] is what microphone k hears later than beam b's time axis.
 *
 * Quantisation (uc_scan_quantise).  A delay is quantised once: q = llrint(d * 256) (ties to even), an int32.  Its
 * coefficients are those of uc_array_tap_coefficients(q / 256.0, weight_k): shift = (q >> 8) - 7, and the sixteen floats
 * are row q & 255 of tap k's table, uc_scan_table(weight_k): row 0 is {c[7] = weight, zeros elsewhere}, row f
 *   c[t] = (float)(weight * sinc(u) * I0(8 * sqrt(1 - (u / 8)^2)) / I0(8)),  u = t - 7 - f / 256,  t = 0 .. 15,
 * evaluated operation for operation as the array combiner's host code does.  The device never evaluates a sinc, and
 * nothing is evaluated per call.
 *
 * Beam sample.  y_b[j] is the Output paragraph of uchirp_array.h for the taps {q_bk / 256, weight_k, mics[k] + a *
 * array_rows}, k ascending:
 *   a_k = c_k[0] * x_k[j + shift_k];  a_k = fmaf(c_k[t], x_k[j + shift_k + t], a_k)  for t = 1 .. 15
 *   y = a_0;  y = y + a_k  for k = 1 .. n_taps - 1      (each addition rounded once)
 * so y is bit for bit what uc_array_combine writes for those taps.
 *
 * Power of (array a, window w, beam b).  The window covers j = first + w * hop + i, i = 0 .. window_len - 1 (hop >= 1;
 * windows may overlap, leave gaps, and reach outside the rows, where they read zeros).  Segments of 4096 samples are
 * counted from the window's first sample.  Within a segment sample i' belongs to chain (i' mod 256) div 4.  Every chain
 * starts at +0.0f and takes its samples ascending: s = y * y (one rounding), a = a + s (one rounding, no fused
 * multiply-add).  The 64 chain sums are added by the tree h = 32, 16, 8, 4, 2, 1 (chain l takes chain l + h, l < h).  The
 * segment sums are converted to double and added from 0.0 in ascending segment order.  The longest path has 71 float
 * roundings.  The double is stored at power_dev[(a * n_windows + w) * power_stride + b]; power_stride 0 means n_beams.
 * A value depends on the inputs, the steering set and the window only, never on the grid, the path the kernel took, the
 * other beams, windows or arrays, or how a recording is cut into calls.
 *
 * Best record.  best_dev[a * n_windows + w]: the beam of greatest power of that row of powers, the lowest index on a tie.
 * If any power of the row is not finite: flags = UC_SCAN_NOT_FINITE, beam = 0, power = 0.0.
 *
 * OUT OF SCOPE: estimating positions beyond the arg-max (no interpolation between candidates); adaptive or data-dependent
 * weights (MVDR, PHAT); per-array steering sets; per-microphone clock offsets (uc_retime_rows, uchirp_retime.h, goes in
 * front); candidate delays finer than 1/256 sample; capture into a graph; more than one GPU per object.
 */
#ifndef UCHIRP_SCAN_H
#define UCHIRP_SCAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UC_SCAN_ABI_VERSION 1

#define UC_SCAN_DTYPE_I32 0 /* DFSDM words */
#define UC_SCAN_DTYPE_F32 1

#define UC_SCAN_MAX_TAPS 32     /* microphones of a steering set */
#define UC_SCAN_COEFS 16        /* coefficients of one tap */
#define UC_SCAN_FRACTIONS 256   /* rows of a tap's table: delays are multiples of 1/256 sample */
#define UC_SCAN_MAX_BEAMS 1048576
#define UC_SCAN_SEGMENT 4096    /* samples of one float32 partial sum */

#define UC_SCAN_NOT_FINITE 1u   /* uc_scan_best.flags: a power of the row is NaN or infinite */

typedef struct uc_scan uc_scan;

/* the strongest beam of one (array, window) (16 bytes) */
typedef struct uc_scan_best {
  uint32_t beam;
  uint32_t flags;
  double power;
} uc_scan_best;

int uc_scan_abi_version(void);
/* text of the calling thread's last error ("" if none) */
const char* uc_scan_last_error(void);
/* -ENODEV ("no CPU path") when no GPU is visible */
int uc_scan_create(int device, uc_scan** out);
/* Waits for the device, and with it for every call of the object on whatever stream it was given (a call that stages
 * nothing leaves no event to wait for), then frees it.  NULL is allowed. */
void uc_scan_destroy(uc_scan* scan);

/* q = llrint(delay_samples * 256); needs no GPU.  -EINVAL: q NULL, delay_samples not finite or |delay_samples| > 2^20. */
int uc_scan_quantise(double delay_samples, int32_t* q);
/* The 256 coefficient rows of a tap of this weight; needs no GPU.  -EINVAL: table NULL, weight not finite. */
int uc_scan_table(float weight, float table[UC_SCAN_FRACTIONS * UC_SCAN_COEFS]);

/* The definition itself in plain C on HOST memory, for ONE beam and ONE window of one array: `in` holds n_rows rows as
 * above, mics[k] < n_rows names tap k's row, q[k] its quantised delay (|q| <= 2^28); *power receives the window's power.
 * Needs no GPU.  -EINVAL: a NULL pointer, an unknown dtype, a zero count, n_taps > UC_SCAN_MAX_TAPS, a mic >= n_rows, a
 * weight that is not finite, |q[k]| > 2^28, in_stride < n_in, a sample range beyond the limits of uc_scan_power. */
int uc_scan_power_row(const void* in, int in_dtype, size_t n_rows, uint64_t in_first, size_t n_in, size_t in_stride,
                      const uint32_t* mics, const float* weights, const int32_t* q, size_t n_taps, uint64_t first,
                      size_t window_len, double* power);

/* Replaces the object's steering set: mics, weights (n_taps each) and delays (n_beams rows of n_taps doubles,
 * delay_stride doubles apart; 0 means n_taps) are HOST arrays.  Synchronous (it waits for the device before
 * it frees the old set, so no call in flight on any stream still reads it), and all or nothing: a refused call
 * (-EINVAL: a NULL pointer, n_taps not in 1 .. UC_SCAN_MAX_TAPS, n_beams not in 1 .. UC_SCAN_MAX_BEAMS, delay_stride <
 * n_taps, a weight or a delay that is not finite, |delay| > 2^20) leaves the old set in place. */
int uc_scan_set_beams(uc_scan* scan, const uint32_t* mics, const float* weights, size_t n_taps, const double* delays,
                      size_t n_beams, size_t delay_stride);

/* How many beams of the uploaded set the kernel takes by its direct path (global loads) because a shift of theirs lies
 * outside the image the kernel stages; the bits are the same on both paths.  -EINVAL: a NULL pointer, no set. */
int uc_scan_direct_beams(const uc_scan* scan, uint32_t* n_direct);

/* Writes the powers of n_arrays x n_windows x n_beams (array, window, beam) triples and / or the best records.  in_dev,
 * power_dev (doubles) and best_dev are device memory of the object's device; either of power_dev, best_dev may be NULL,
 * not both; with power_dev NULL the powers live in the object's scratch.  in_stride 0 means n_in, power_stride 0 means
 * n_beams.  `first` is the absolute sample of window 0.  Asynchronous on hip_stream (a hipStream_t, or NULL); the caller's
 * current HIP device is restored.  Every argument is checked and every buffer is sized before anything is enqueued: a
 * refused call (negative errno) has enqueued nothing and leaves the object usable.  -EINVAL: a NULL scan or in_dev, both
 * outputs NULL; a zero count (n_rows, n_in, n_arrays, array_rows, window_len, hop, n_windows) or an unknown dtype; no
 * steering set; a mic of the set >= array_rows; n_arrays * array_rows > n_rows; in_stride < n_in, power_stride < n_beams;
 * in_first or first > 2^52, n_in, window_len, hop, a stride > 2^40, first + n_windows * hop + window_len > 2^53; more than
 * 2^32 - 1 triples; a pointer that is not device memory of the object's device, in_dev not on 4 bytes, power_dev or
 * best_dev not on 8; outputs overlapping the input or each other.  One thread at a time per object; not capturable into
 * a graph. */
int uc_scan_power(uc_scan* scan, const void* in_dev, int in_dtype, size_t n_rows, uint64_t in_first, size_t n_in,
                  size_t in_stride, size_t n_arrays, size_t array_rows, uint64_t first, size_t window_len, size_t hop,
                  size_t n_windows, double* power_dev, size_t power_stride, uc_scan_best* best_dev, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
