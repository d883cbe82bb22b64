/* uchirp_xcorr.h -- C-ABI of libuchirp_xcorr.so: the wide-lag correlator of the chirp modem (cross-correlation of array
 * microphones with a reference microphone out to +-512 lags by overlap-save FFT, and the crest rule that turns a
 * correlation into a fractional delay).
 *
 * uc_align_correlate (uchirp_align.h) evaluates lags directly and stops at +-64 samples: 0.82 ms at 78 125 samples/s,
 * about 28 cm of path difference.  Microphones spread over a room, or a recording that arrives milliseconds late, need
 * more.  This library computes the same sums r_p[l] for l = -L .. L, L up to 512, through 2048-point transforms whose
 * cost does not grow with L.
 *
 * The library stands alone: it needs no symbol of libuchirp.so, libuchirp_link.so, libuchirp_scene.so, libuchirp_array.so
 * or libuchirp_align.so.  There is no CPU path: uc_xcorr_create fails without a GPU.  uc_xcorr_peak is pure host
 * arithmetic and works anywhere.
 *
 * DEFINITION OF THE CORRELATION
 *
 * Input.  n_mics rows in device memory, UC_XCORR_DTYPE_F32 (float) or UC_XCORR_DTYPE_I32 (DFSDM words, each cast with
 * (float) as the receivers do).  Row m starts at in_dev + m * in_stride (elements) and holds n_in samples.  x_m[j] is
 * sample j of row m after the cast; a sample of the MICROPHONE row outside [0, n_in) reads as +0.0f (the reference row is
 * only read inside [first, first + n), which lies inside the row).
 *
 * Pair.  { ref, mic }: two rows (they may be the same row).  With L = max_lag, for l = -L .. L
 *   r_p[l] = sum over j = first .. first + n - 1 of  x_ref[j] * x_mic[j + l]
 * is stored as a double at corr_dev[p * corr_stride + (l + L)].  A positive lag of the crest means that the microphone
 * hears the sound LATER than the reference: it is the delay_samples of uc_array_tap against the reference.
 *
 * How it is computed.  P = UC_XCORR_POINTS = 2048 and S = P - 2 L.  Segment s holds the reference samples
 * i = s S .. min(s S + S - 1, n - 1), counted from first; cnt is its length.
 *   a_s[t] = x_ref[first + s S + t]       for t < cnt,        else +0.0f
 *   b_s[t] = x_mic[first + s S - L + t]   for t < cnt + 2 L,  else +0.0f      (t = 0 .. P - 1)
 * The circular correlation c_s[t] = sum over i of a_s[i] * b_s[(i + t) mod P] of length P equals the linear one for
 * t = 0 .. 2 L, which is lag t - L: nothing wraps because i + t <= P - 1 wherever a_s[i] is not zero.  It is evaluated in
 * float as inverse transform(conj(A_s) * B_s), with A_s and B_s the P-point transforms of a_s and b_s.
 * UC_XCORR_GROUP = G = 4 consecutive segments form a group: the cross-spectra conj(A_s) * B_s of a group are added in
 * float, bin by bin, in ascending segment order, and ONE inverse transform per group yields the 2 L + 1 float UNIT SUMS of
 * the group.  The unit sums are converted to double and added in double, starting from 0.0, in ascending group order.
 * A result depends on the inputs, the pair, first, n and L only: never on the grid, on which workgroup handled which
 * group, on the other pairs of the call or on their order.
 *
 * Non-finite samples.  One float sample x_m[q] that is NaN, +Inf or -Inf (integer words hold none):
 *   MUST      r_p[l] is not finite wherever its sum has a term with x_m[q]: for every l if m is the pair's reference row and
 *             first <= q < first + n (also where the other factor is a microphone sample outside the row, +0.0f); for the
 *             lags with first <= q - l < first + n if m is the pair's microphone row.
 *   MAY       the other lags of such a pair: the 2 L + 1 sums of a group come out of one inverse transform, so a pair that
 *             has one MUST lag may be not finite at all its lags (this implementation: it is).  Such a value is either
 *             bit for bit the clean call's or not finite, never another finite number.
 *   MUST NOT  everything else the call writes -- the pairs that read row m only outside the reference's
 *             [first, first + n) and the microphone's [first - L, first + n + L), all other pairs, and every word of
 *             corr_dev between the rows -- is bit for bit what the same call writes with a finite sample there.
 * uc_xcorr_peak refuses a correlation with a value that is not finite (-EINVAL): it is the host's detector.
 *
 * Error.  With E_p = sum over s of ||a_s||_2 * ||b_s||_2 (Euclidean norms; no product of a segment can exceed its term),
 *   |r_p[l] - exact| <= UC_XCORR_ERROR_C * 2^-24 * E_p.
 * The constant is measured, not derived: four times the worst ratio an independent float32 evaluation of the same
 * definition reaches on the test inputs, rounded up.
 *
 * DEFINITION OF THE PEAK (uc_xcorr_peak; double arithmetic on the host)
 *
 * The rule of uchirp_align.h, word for word.  With r[k], k = 0 .. 2L, the values for l = k - L:
 *   a candidate is every k in 1 .. 2L - 1 with r[k] > 0, r[k] >= r[k-1] and r[k] > r[k+1];
 *   c = (r[k-1] + r[k+1]) / (2 r[k]);
 *   if -1 < c < 1:  w = acos(c),  q = (r[k+1] - r[k-1]) / (2 sin w),  height = hypot(r[k], q),  d = atan2(q, r[k]) / w
 *   otherwise       height = r[k],  d = 0;
 *   the estimate is the candidate of greatest height, the first one on a tie.
 *
 * OUT OF SCOPE: PHAT or other spectral weightings; lag ranges beyond UC_XCORR_MAX_LAG; tracking delays over time; capture
 * into a graph; resolving whole-cycle ambiguity at low SNR beyond reporting runner_up.  Fixed spectral weights (the chirps'
 * band), which keep the crest on its cycle at low SNR: uchirp_wcorr.h.
 */
#ifndef UCHIRP_XCORR_H
#define UCHIRP_XCORR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UC_XCORR_ABI_VERSION 1

#define UC_XCORR_DTYPE_I32 0 /* DFSDM words */
#define UC_XCORR_DTYPE_F32 1

#define UC_XCORR_MAX_LAG 512 /* L = max_lag is 1 .. 512 */
#define UC_XCORR_POINTS 2048 /* P: length of the transforms; a segment holds S = P - 2 L reference samples */
#define UC_XCORR_GROUP 4     /* G: segments whose cross-spectra are added in float before one inverse transform */
#define UC_XCORR_ERROR_C 11  /* C of the error form */

#define UC_XCORR_NO_PEAK 1u /* flags: no candidate; delay_samples, height, lag and runner_up are 0 */
#define UC_XCORR_AT_EDGE 2u /* flags: the largest sample of r lies at index 0 or 2L: the true crest may lie outside */

typedef struct uc_xcorr uc_xcorr;

/* one pair of rows (8 bytes) */
typedef struct uc_xcorr_pair {
  uint32_t ref; /* row of the reference microphone (< n_mics) */
  uint32_t mic; /* row of the microphone (< n_mics) */
} uc_xcorr_pair;

/* what uc_xcorr_peak reads off one correlation (32 bytes; the layout of uc_align_peak_t) */
typedef struct uc_xcorr_peak_t {
  double delay_samples; /* k - L + d of the chosen candidate */
  double height;        /* its fitted height */
  double runner_up;     /* second-greatest candidate height / height, 0 with one candidate */
  int32_t lag;          /* k - L */
  uint32_t flags;       /* UC_XCORR_NO_PEAK | UC_XCORR_AT_EDGE */
} uc_xcorr_peak_t;

int uc_xcorr_abi_version(void);
/* text of the calling thread's last error ("" if none) */
const char* uc_xcorr_last_error(void);
/* -ENODEV ("no CPU path") when no GPU is visible */
int uc_xcorr_create(int device, uc_xcorr** out);
/* Waits for every call of the object still in flight, on whatever streams they were given (each call is ordered behind the
 * call two before it, so the events of the last two cover all), then frees it.  NULL is allowed. */
void uc_xcorr_destroy(uc_xcorr* xcorr);

/* The correlations of the definition for n_pairs pairs.  pairs is a HOST array: it is copied, with the records derived
 * from it, into one of two pinned staging buffers of the object, used in turn, before the call returns (the caller may
 * reuse it at once), and from there to the device on hip_stream.  in_dev and corr_dev are device memory of the object's
 * device; strides are in elements (of the input's type, of double), 0 means the count (n_in, 2 max_lag + 1).  Only the
 * 2 max_lag + 1 doubles of every row of corr_dev are written.  Asynchronous on hip_stream (a hipStream_t, or NULL); the
 * caller's current HIP device is restored.  Every argument is checked and every buffer is sized before anything is
 * enqueued: a refused call (negative errno) has enqueued nothing and leaves the object usable.  -EINVAL: a pair's ref or
 * mic >= n_mics; first + n > n_in; max_lag not in 1 .. UC_XCORR_MAX_LAG; corr_stride < 2 max_lag + 1 (unless 0);
 * in_stride < n_in (unless 0); a zero count (n_mics, n_in, n_pairs, n); an unknown dtype; a NULL array; in_dev or
 * corr_dev not device memory of the object's device; corr_dev overlapping in_dev.  One thread at a time per object; not
 * capturable into a graph. */
int uc_xcorr_correlate(uc_xcorr* xcorr, const void* in_dev, int in_dtype, size_t n_mics, size_t n_in, size_t in_stride,
                       const uc_xcorr_pair* pairs, size_t n_pairs, size_t first, size_t n, uint32_t max_lag, double* corr_dev,
                       size_t corr_stride, void* hip_stream);

/* The peak of the definition over corr[0 .. 2 max_lag] (HOST memory); needs no GPU.  -EINVAL: a NULL pointer, max_lag
 * not in 1 .. UC_XCORR_MAX_LAG, a value that is not finite. */
int uc_xcorr_peak(const double* corr, uint32_t max_lag, uc_xcorr_peak_t* out);

#ifdef __cplusplus
}
#endif
#endif
