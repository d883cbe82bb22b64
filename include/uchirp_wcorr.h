/* uchirp_wcorr.h -- C-ABI of libuchirp_wcorr.so: the band-weighted correlator of the chirp modem (the windowed
 * cross-correlations of uchirp_track.h with a real weight on every bin of the 2048-point cross-spectrum, so that only the
 * band the chirps occupy adds to a sum, and the crest rule that turns a correlation into a fractional delay).
 *
 * uc_align_correlate, uc_xcorr_correlate and uc_track_windows correlate the rows as they come, over the whole band 0 ..
 * 39 kHz, while the chirps occupy 16 .. 19 kHz: most of what those sums add up is noise times noise from outside the
 * band, and at low SNR the crest rule then lands on a neighbouring crest of the 17.5 kHz carrier, 4.46 samples off.
 * Weights of 1 on the band with cos^2 edges keep the crest on the right carrier cycle (DESIGN.md section 20 has the
 * figures).  The weights cost sixteen multiplies per thread and unit and no pass over the samples.
 *
 * The library stands alone: it needs no symbol of the other eleven libraries.  There is no CPU path: uc_wcorr_create
 * fails without a GPU.  uc_wcorr_band_weights and uc_wcorr_peak are pure host arithmetic and work anywhere.
 *
 * DEFINITION OF THE CORRELATION of (pair p, window w)
 *
 * Input.  n_mics rows in device memory, UC_WCORR_DTYPE_F32 (float) or UC_WCORR_DTYPE_I32 (DFSDM words, each cast with
 * (float) as the receivers do).  Row m starts at in_dev + m * in_stride (elements) and holds n_in samples.  x_m[j] is
 * sample j of row m after the cast; a sample of the MICROPHONE row outside [0, n_in) reads as +0.0f (the reference row is
 * only read inside its windows, which lie inside the row).
 *
 * Pair.  { ref, mic }: two rows (they may be the same row).  A positive lag means that the microphone hears the sound
 * LATER than the reference: it is the delay_samples of uc_array_tap against the reference.
 *
 * Windows.  Window w = 0 .. n_windows - 1 covers the reference samples [first + w hop, first + w hop + window_len).
 * hop >= 1; hop < window_len (the windows overlap) and hop > window_len (gaps between them) are both allowed;
 * window_len >= 1; first + (n_windows - 1) hop + window_len <= n_in.  One window is the uc_xcorr_correlate case.
 *
 * Weights.  A HOST array of UC_WCORR_BINS = 1025 finite floats w[k] for the bins k = 0 .. 1024 of the 2048-point transform
 * (bin k is the frequency k fs / 2048); NULL means all ones.  The full table is W[k] = w[k] for k <= 1024 and
 * W[k] = w[2048 - k] above: real and even, so the weighted correlation stays real.
 *
 * Guard.  guard extra lags on either side that are computed and not stored.  With L = max_lag and L' = L + guard:
 * 1 <= L and L' <= UC_WCORR_MAX_LAG = 512.
 *
 * How it is computed.  The segments, the groups and every transform are exactly those of uchirp_xcorr.h AT max_lag = L',
 * over the window first' = first + w hop, n' = window_len.  P = UC_WCORR_POINTS = 2048 and S = P - 2 L'.  Segment s holds
 * the reference samples i = s S .. min(s S + S - 1, n' - 1), counted from first'; cnt is its length.
 *   a_s[t] = x_ref[first' + s S + t]        for t < cnt,         else +0.0f
 *   b_s[t] = x_mic[first' + s S - L' + t]   for t < cnt + 2 L',  else +0.0f      (t = 0 .. P - 1)
 * A_s and B_s are the P-point transforms of a_s and b_s, evaluated in float.  UC_WCORR_GROUP = G = 4 consecutive
 * segments form a group: the cross-spectra conj(A_s) * B_s of a group are added in float, bin by bin, in ascending
 * segment order.  EACH OF THE 2048 BINS OF THAT SUM IS THEN MULTIPLIED BY W[k]: one float multiply for the real part and
 * one for the imaginary part.  ONE inverse transform per group and the factor 2^-11 yield c[t], t = 0 .. P - 1; t is lag
 * t - L'.  Of the 2 L' + 1 values c[0 .. 2 L'] those with index guard .. guard + 2 L (the lags -L .. L) are the group's
 * UNIT SUMS.  The unit sums are converted to double and added in double, starting from 0.0, in ascending group order, and
 * stored at
 *   corr_dev[(p * n_windows + w) * corr_stride + (l + L)],   l = -L .. L.
 *
 * What that is.  With c_s[t] = sum over i of a_s[i] * b_s[(i + t) mod P] the circular correlation of a segment and
 *   h[t] = (1 / 2048) * sum over k = 0 .. 2047 of W[k] cos(2 pi k t / 2048)
 * the weights' impulse response (real and even), the model of a stored value is
 *   r[l] = sum over the window's segments s of  sum over u = 0 .. P - 1 of  h[u] * c_s[(l + L' - u) mod P]:
 * the circular convolution of every segment's 2048-point correlation with h.  This is the definition, and it is total.
 * c_s[t] is the linear correlation of lag t - L' for t = 0 .. 2 L' only; the other 2047 - 2 L' values of c_s wrap.  A
 * stored lag draws on them with the weights h[u], |u| > guard (circular distance), so that with T(guard) the share of
 * h's energy at circular distance > guard (*tail_out of uc_wcorr_band_weights) the distance to the ideal, linearly
 * filtered correlation is bounded by the tail of h: for the band 16 .. 19 kHz with 1 kHz edges at fs = 78 125 Hz,
 *   guard      0       32       64       128      256
 *   T(guard)   0.89    1.6e-2   1.8e-3   1.8e-5   3.6e-7
 * and the largest deviation from the ideal, as a share of the peak at -12 dB, had a median of 5e-3 at guard 0 and of 7e-5
 * at guard 128.  RECOMMENDED: guard = 128 (max_lag <= 384 with it).
 *
 * Bit contract.  A result depends on the inputs, the pair, the window, L, guard and the weights only: never on the grid,
 * on which workgroup handled which group, on the other pairs or windows of the call, on their order or on how a series is
 * cut into calls.  weights NULL and an explicit table of ones give the same bits; with guard 0 these are the bits of
 * uc_track_windows' correlations and of uc_xcorr_correlate, and with guard g the central 2 L + 1 values of
 * uc_xcorr_correlate at max_lag L + g.  Weights scaled by a power of two scale every result exactly (short of underflow
 * and overflow).  Weights of zero give 0.0 for finite inputs.
 *
 * Non-finite samples.  One float sample x_m[q] that is NaN, +Inf or -Inf (integer words hold none).  The definition
 * above is total: a stored lag is a sum over every segment's whole 2048-point correlation, so every sample of a segment
 * has a term in every stored lag of its (pair, window), whatever its coefficient h[u] -- with weights of ones h is the
 * unit impulse and most of these coefficients are zero, with weights of zero all are: 0 * NaN is NaN, and the 0.0 of
 * weights of zero becomes NaN.  With first' = first + w hop, n' = window_len and L' = max_lag + guard:
 *   MUST      all 2 max_lag + 1 stored values of (pair, window) are not finite if m is the pair's reference row and
 *             first' <= q < first' + n', or its microphone row and first' - L' <= q < first' + n' + L': the guard widens
 *             the microphone's range, although its lags are not stored.
 *   MAY       nothing.
 *   MUST NOT  every other (pair, window) -- with overlapping windows a sample lies in several, with gaps it may lie in
 *             none -- and every word of corr_dev between the rows: bit for bit what the same call writes with a finite
 *             sample there.
 * uc_wcorr_peak refuses a correlation with a value that is not finite (-EINVAL): it is the host's detector.
 *
 * Error.  With E_p = sum over s of ||a_s||_2 * ||b_s||_2 as in uchirp_xcorr.h at L',
 *   |r[l] - model| <= UC_WCORR_ERROR_C * 2^-24 * max_k |w[k]| * E_p.
 * The constant is measured by that header's recipe, not derived: four times the worst ratio an independent float32
 * evaluation of the same definition (uchirp/wcorr.py, emulate32) reaches on the test inputs, rounded up (DESIGN.md
 * section 20).  It is not the GPU's own error.
 *
 * DEFINITION OF THE BAND WEIGHTS (uc_wcorr_band_weights; double arithmetic on the host)
 *
 * With f_k = k fs / 2048, k = 0 .. 1024: w[k] = 1 for f_lo <= f_k <= f_hi; outside the band, at the distance
 * d = f_lo - f_k or f_k - f_hi, w[k] = cos^2(pi / 2 * d / taper_hz) for d < taper_hz and 0 beyond; taper_hz = 0 is a brick
 * wall.  Computed in double and rounded to float.  T(guard) is computed in double from the ROUNDED weights: the sum of
 * h[t]^2 over the t = 0 .. 2047 with min(t, 2048 - t) > guard, over the sum of all h[t]^2 (0 if that is 0); it is exactly
 * 0 for guard >= 1024.
 *
 * DEFINITION OF THE PEAK (uc_wcorr_peak; double arithmetic on the host)
 *
 * The rule of uchirp_xcorr.h (that of uchirp_align.h), word for word and with the same bits as uc_xcorr_peak.  With r[k],
 * k = 0 .. 2L, the values for l = k - L:
 *   a candidate is every k in 1 .. 2L - 1 with r[k] > 0, r[k] >= r[k-1] and r[k] > r[k+1];
 *   c = (r[k-1] + r[k+1]) / (2 r[k]);
 *   if -1 < c < 1:  w = acos(c),  q = (r[k+1] - r[k-1]) / (2 sin w),  height = hypot(r[k], q),  d = atan2(q, r[k]) / w
 *   otherwise       height = r[k],  d = 0;
 *   the estimate is the candidate of greatest height, the first one on a tie.
 *
 * OUT OF SCOPE: PHAT and any weight that depends on the data (it needs a window's whole cross-spectrum before the
 * inverse transform, which is another deal); the analytic envelope (measured, it adds nothing to the crest rule on the
 * weighted correlation); crest records on the device (the tracker's second kernel); L' beyond UC_WCORR_MAX_LAG; making
 * this library the default of uc_align, uc_xcorr, uc_track or the retimer's drift estimate; capture into a graph.
 */
#ifndef UCHIRP_WCORR_H
#define UCHIRP_WCORR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UC_WCORR_ABI_VERSION 1

#define UC_WCORR_DTYPE_I32 0 /* DFSDM words */
#define UC_WCORR_DTYPE_F32 1

#define UC_WCORR_MAX_LAG 512 /* L' = max_lag + guard is at most 512; max_lag >= 1 */
#define UC_WCORR_POINTS 2048 /* P: length of the transforms; a segment holds S = P - 2 L' reference samples */
#define UC_WCORR_GROUP 4     /* G: segments whose cross-spectra are added in float before one inverse transform */
#define UC_WCORR_BINS 1025   /* weights: the bins 0 .. P / 2 */
#define UC_WCORR_ERROR_C 9   /* C of the error form */

#define UC_WCORR_NO_PEAK 1u /* flags: no candidate; delay_samples, height, lag and runner_up are 0 */
#define UC_WCORR_AT_EDGE 2u /* flags: the largest sample of r lies at index 0 or 2L: the true crest may lie outside */

typedef struct uc_wcorr uc_wcorr;

/* one pair of rows (8 bytes; the layout of uc_xcorr_pair) */
typedef struct uc_wcorr_pair {
  uint32_t ref; /* row of the reference microphone (< n_mics) */
  uint32_t mic; /* row of the microphone (< n_mics) */
} uc_wcorr_pair;

/* what uc_wcorr_peak reads off one correlation (32 bytes; the layout of uc_xcorr_peak_t) */
typedef struct uc_wcorr_peak_t {
  double delay_samples; /* k - L + d of the chosen candidate */
  double height;        /* its fitted height */
  double runner_up;     /* second-greatest candidate height / height, 0 with one candidate */
  int32_t lag;          /* k - L */
  uint32_t flags;       /* UC_WCORR_NO_PEAK | UC_WCORR_AT_EDGE */
} uc_wcorr_peak_t;

int uc_wcorr_abi_version(void);
/* text of the calling thread's last error ("" if none) */
const char* uc_wcorr_last_error(void);
/* -ENODEV ("no CPU path") when no GPU is visible */
int uc_wcorr_create(int device, uc_wcorr** out);
/* Waits for every call of the object still in flight, on whatever streams they were given (each call is ordered behind the
 * call two before it, so the events of the last two cover all), then frees it.  NULL is allowed. */
void uc_wcorr_destroy(uc_wcorr* wcorr);

/* The correlations of the definition for n_pairs pairs and n_windows windows.  pairs and weights are HOST arrays: they are
 * copied, with the records derived from the pairs, into one of two pinned staging buffers of the object, used in turn,
 * before the call returns (the caller may reuse them at once), and from there to the device on hip_stream.  weights may
 * be NULL (all ones).  in_dev and corr_dev are device memory of the object's device.  Strides are in elements (of the
 * input's type, of double), 0 means the count (n_in, 2 max_lag + 1).  Only the 2 max_lag + 1 doubles of every row of
 * corr_dev are written.  Asynchronous on hip_stream (a hipStream_t, or NULL); the caller's current HIP device is restored.
 * Every argument is checked and every buffer (the unit sums included) is sized before anything is enqueued: a refused call
 * (negative errno) has enqueued nothing and leaves the object usable.
 * -EINVAL: a pair's ref or mic >= n_mics; hop = 0; a window past n_in (first + (n_windows - 1) hop + window_len > n_in);
 * max_lag = 0; max_lag + guard > UC_WCORR_MAX_LAG; a weight that is not finite; corr_stride < 2 max_lag + 1 (unless 0);
 * in_stride < n_in (unless 0); a zero count (n_mics, n_in, n_pairs, window_len, n_windows); an unknown dtype; a NULL array
 * (weights excepted); in_dev or corr_dev not device memory of the object's device; corr_dev overlapping in_dev; more than
 * 2^32 - 1 units (n_pairs * n_windows * groups of a window) in one call.  -ENOMEM: the scratch (staging, unit sums) cannot
 * be had.  One thread at a time per object; not capturable into a graph. */
int uc_wcorr_windows(uc_wcorr* wcorr, const void* in_dev, int in_dtype, size_t n_mics, size_t n_in, size_t in_stride,
                     const uc_wcorr_pair* pairs, size_t n_pairs, size_t first, size_t window_len, size_t hop,
                     size_t n_windows, uint32_t max_lag, uint32_t guard, const float* weights, double* corr_dev,
                     size_t corr_stride, void* hip_stream);

/* The band weights of the definition into w_out[0 .. 1024] (HOST memory), and into *tail_out (unless NULL) the share
 * T(guard) of their impulse response's energy; needs no GPU.  -EINVAL: w_out NULL; a value that is not finite; fs <= 0;
 * f_lo < 0; f_lo > f_hi; taper_hz < 0. */
int uc_wcorr_band_weights(double fs, double f_lo, double f_hi, double taper_hz, uint32_t guard, float* w_out, double* tail_out);

/* The peak of the definition over corr[0 .. 2 max_lag] (HOST memory); needs no GPU.  -EINVAL: a NULL pointer, max_lag
 * not in 1 .. UC_WCORR_MAX_LAG, a value that is not finite. */
int uc_wcorr_peak(const double* corr, uint32_t max_lag, uc_wcorr_peak_t* out);

#ifdef __cplusplus
}
#endif
#endif
