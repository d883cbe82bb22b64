/* uchirp_track.h -- C-ABI of libuchirp_track.so: the delay tracker of the chirp modem (the cross-correlations of
 * uchirp_xcorr.h over a SERIES OF WINDOWS of one recording in one call, and a crest search on the device that leaves one
 * small record per (pair, window) for the host to finish).
 *
 * uc_xcorr_correlate (uchirp_xcorr.h) and uc_align_correlate (uchirp_align.h) give one correlation per pair and call, and
 * both list "tracking delays over time" as out of scope: a moving transmitter, or a microphone whose clock drifts, needs a
 * delay per (pair, window), and getting it from them costs one call, one copy of every pair's 2 L + 1 doubles and one
 * host peak search per window.  This library does all windows in one call and copies 136 bytes per (pair, window).
 *
 * The library stands alone: it needs no symbol of the other seven libraries.  There is no CPU path: uc_track_create fails
 * without a GPU.  uc_track_finish is pure host arithmetic and works anywhere.
 *
 * WINDOWS
 *
 * Window w = 0 .. n_windows - 1 covers the reference samples [first + w hop, first + w hop + window_len).  hop >= 1;
 * hop < window_len (the windows overlap) and hop > window_len (gaps between them) are both allowed; window_len >= 1;
 * first + (n_windows - 1) hop + window_len <= n_in.
 *
 * DEFINITION OF THE CORRELATION of (pair p, window w)
 *
 * By definition what uc_xcorr_correlate (uchirp_xcorr.h, DEFINITION OF THE CORRELATION) gives for that pair with
 * first' = first + w hop, n' = window_len and the same max_lag = L: the same segments of S = 2048 - 2 L reference samples
 * counted from the window's first sample, the same zero padding, a microphone sample outside [0, n_in) reads +0.0f, groups
 * of G = 4 segments whose cross-spectra are added in float in ascending order, one inverse transform per group (unit sums
 * times 2^-11), the unit sums added in double from 0.0 in ascending group order.  Rows are UC_TRACK_DTYPE_F32 or
 * UC_TRACK_DTYPE_I32 (cast with (float)).  A result depends on the inputs, the pair, the window and L only: never on the
 * grid, on the other pairs or windows of the call or on their order.  It is stored as doubles at
 *   corr_dev[(p * n_windows + w) * corr_stride + (l + L)],   l = -L .. L.
 * The arithmetic is that of uc_xcorr_correlate, so its error form carries over with UC_XCORR_ERROR_C = 11:
 *   |r[l] - exact| <= 11 * 2^-24 * E_p,   E_p = sum over the window's segments of ||a_s||_2 ||b_s||_2.
 *
 * Non-finite samples.  One float sample x_m[q] that is NaN, +Inf or -Inf (integer words hold none); per (pair, window),
 * with first' = first + w hop and n' = window_len, the zones of uchirp_xcorr.h:
 *   MUST      r[l] is not finite wherever its sum has a term with x_m[q]: every l if m is the pair's reference row and
 *             first' <= q < first' + n'; the lags with first' <= q - l < first' + n' if m is its microphone row.  The crest
 *             record of such a (pair, window) has flags == UC_TRACK_NOT_FINITE alone and every other byte zero, and
 *             uc_track_finish refuses it (-EINVAL): flags is the caller's test, on the device's record or on the host.
 *   MAY       the other lags of such a (pair, window): its sums come out of one inverse transform per group (this
 *             implementation: they are all not finite).  Each is bit for bit the clean call's or not finite.
 *   MUST NOT  every (pair, window) that reads row m only outside the reference's [first', first' + n') and the
 *             microphone's [first' - L, first' + n' + L) -- with overlapping windows a sample lies in several, with gaps
 *             it may lie in none --, their crest records, and every word of corr_dev between the rows: bit for bit what
 *             the same call writes with a finite sample there.
 *
 * DEFINITION OF THE CREST RECORD (uc_track_crest; written by the device at crest_dev[p * n_windows + w])
 *
 * With r[k], k = 0 .. 2L, the doubles of one correlation:
 *   flags         UC_TRACK_NO_PEAK and UC_TRACK_AT_EDGE with the meaning of UC_XCORR_NO_PEAK and UC_XCORR_AT_EDGE (no
 *                 candidate; the largest sample, the first one on a tie, lies at index 0 or 2L).  UC_TRACK_NOT_FINITE: some
 *                 r[k] is not finite; every other byte of the record is then zero.
 *   n_candidates  the number of k in 1 .. 2L - 1 with r[k] > 0, r[k] >= r[k-1] and r[k] > r[k+1] (the candidates of
 *                 uc_xcorr_peak)
 *   slot[4]       { k, r[k-1], r[k], r[k+1] } of the UC_TRACK_SLOTS = 4 candidates of greatest SELECTION HEIGHT, in
 *                 ascending k; an unused slot has k = -1 and zeros.
 * Selection height h2 of candidate k, in correctly rounded double operations, each rounded once, none contracted:
 *   c = (r[k-1] + r[k+1]) / (2 * r[k])
 *   if -1 < c < 1:  s = sqrt((1 - c) * (1 + c)),  q = (r[k+1] - r[k-1]) / (2 * s),  h2 = r[k] * r[k] + q * q
 *   otherwise       h2 = r[k] * r[k]
 * The greater h2 wins, the smaller k on equal h2.  This is the squared height of uc_xcorr_peak without acos, sin and
 * hypot, whose last bits differ between device and host libraries: it only has to bring the true best two into four slots.
 *
 * FINISHING (uc_track_finish; double arithmetic on the host)
 *
 * The loop body of uc_xcorr_peak (acos, sin, hypot, atan2; the first candidate on a tie) over the occupied slots in
 * ascending k.  The finished record equals uc_xcorr_peak of the same 2 L + 1 doubles bit for bit whenever that function's
 * best and second-best candidates are among the four slots, which fails only if three other candidates come within
 * rounding error of them.
 *
 * OUT OF SCOPE: fitting lines to the delays on the GPU; PHAT or other spectral weightings; lag ranges beyond
 * UC_TRACK_MAX_LAG; capture into a graph; resolving whole-cycle ambiguity at low SNR beyond reporting runner_up.  Fixed
 * spectral weights (the chirps' band), which keep the crest on its cycle at low SNR: uchirp_wcorr.h.
 */
#ifndef UCHIRP_TRACK_H
#define UCHIRP_TRACK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UC_TRACK_ABI_VERSION 1

#define UC_TRACK_DTYPE_I32 0 /* DFSDM words */
#define UC_TRACK_DTYPE_F32 1

#define UC_TRACK_MAX_LAG 512 /* L = max_lag is 1 .. 512 */
#define UC_TRACK_POINTS 2048 /* length of the transforms; a segment holds S = 2048 - 2 L reference samples */
#define UC_TRACK_GROUP 4     /* segments whose cross-spectra are added in float before one inverse transform */
#define UC_TRACK_SLOTS 4     /* candidates a crest record keeps */

#define UC_TRACK_NO_PEAK 1u    /* flags: no candidate */
#define UC_TRACK_AT_EDGE 2u    /* flags: the largest sample of r lies at index 0 or 2L */
#define UC_TRACK_NOT_FINITE 4u /* flags (crest record only): some r[k] is not finite; the record is otherwise zero */

typedef struct uc_track uc_track;

/* one pair of rows (8 bytes; the layout of uc_xcorr_pair) */
typedef struct uc_track_pair {
  uint32_t ref; /* row of the reference microphone (< n_mics) */
  uint32_t mic; /* row of the microphone (< n_mics) */
} uc_track_pair;

/* one candidate of a crest record (32 bytes) */
typedef struct uc_track_slot {
  int32_t k;        /* index of the candidate in r (lag k - L), -1: unused */
  int32_t reserved; /* 0 */
  double r[3];      /* r[k-1], r[k], r[k+1] */
} uc_track_slot;

/* what the device leaves of one correlation (136 bytes) */
typedef struct uc_track_crest {
  uint32_t flags;        /* UC_TRACK_NO_PEAK | UC_TRACK_AT_EDGE, or UC_TRACK_NOT_FINITE alone */
  uint32_t n_candidates; /* all candidates of the row, kept or not */
  uc_track_slot slot[UC_TRACK_SLOTS];
} uc_track_crest;

/* what uc_track_finish makes of a crest record (32 bytes; the layout of uc_xcorr_peak_t) */
typedef struct uc_track_peak_t {
  double delay_samples; /* k - L + d of the chosen candidate */
  double height;        /* its fitted height */
  double runner_up;     /* second-greatest candidate height / height, 0 with one candidate */
  int32_t lag;          /* k - L */
  uint32_t flags;       /* UC_TRACK_NO_PEAK | UC_TRACK_AT_EDGE */
} uc_track_peak_t;

int uc_track_abi_version(void);
/* text of the calling thread's last error ("" if none) */
const char* uc_track_last_error(void);
/* -ENODEV ("no CPU path") when no GPU is visible */
int uc_track_create(int device, uc_track** out);
/* Waits for every call of the object still in flight, on whatever streams they were given (each call is ordered behind the
 * call two before it, so the events of the last two cover all), then frees it.  NULL is allowed. */
void uc_track_destroy(uc_track* track);

/* The correlations and crest records of the definitions for n_pairs pairs and n_windows windows.  pairs is a HOST array: it
 * is copied, with the records derived from it, into one of two pinned staging buffers of the object, used in turn, before
 * the call returns (the caller may reuse it at once), and from there to the device on hip_stream.  in_dev, corr_dev and
 * crest_dev are device memory of the object's device; corr_dev or crest_dev may be NULL (not both): what is NULL is not
 * produced.  Strides are in elements (of the input's type, of double), 0 means the count (n_in, 2 max_lag + 1).  Only the
 * 2 max_lag + 1 doubles of every row of corr_dev are written.  Asynchronous on hip_stream (a hipStream_t, or NULL); the
 * caller's current HIP device is restored.  Every argument is checked and every buffer (the unit sums included) is sized
 * before anything is enqueued: a refused call (negative errno) has enqueued nothing and leaves the object usable.
 * -EINVAL: a pair's ref or mic >= n_mics; hop = 0; a window past n_in (first + (n_windows - 1) hop + window_len > n_in);
 * max_lag not in 1 .. UC_TRACK_MAX_LAG; corr_stride < 2 max_lag + 1 (unless 0); in_stride < n_in (unless 0); a zero count
 * (n_mics, n_in, n_pairs, window_len, n_windows); an unknown dtype; a NULL array; both outputs NULL; in_dev, corr_dev or
 * crest_dev not device memory of the object's device; corr_dev overlapping in_dev; crest_dev overlapping in_dev or
 * corr_dev; more than 2^32 - 1 units (n_pairs * n_windows * groups of a window) in one call.  -ENOMEM: the scratch
 * (staging, unit sums) cannot be had.  One thread at a time per object; not capturable into a graph.
 * Test hook, no part of the contract: an object created with UC_TUNING=1 and UC_TRACK_CRESTS_OF_CORR=1 in the environment
 * READS corr_dev (it must be given, as must crest_dev) and runs the crest search alone, so that tests can feed it crafted
 * correlations.  Without UC_TUNING=1 the variable is not looked at. */
int uc_track_windows(uc_track* track, const void* in_dev, int in_dtype, size_t n_mics, size_t n_in, size_t in_stride,
                     const uc_track_pair* pairs, size_t n_pairs, size_t first, size_t window_len, size_t hop,
                     size_t n_windows, uint32_t max_lag, double* corr_dev, size_t corr_stride, uc_track_crest* crest_dev,
                     void* hip_stream);

/* The finished record of one crest record (HOST memory); needs no GPU.  -EINVAL: a NULL pointer, max_lag not in
 * 1 .. UC_TRACK_MAX_LAG, a record that carries UC_TRACK_NOT_FINITE (as uc_xcorr_peak answers a value that is not finite),
 * a slot whose k is neither -1 nor in 1 .. 2 max_lag - 1. */
int uc_track_finish(const uc_track_crest* crest, uint32_t max_lag, uc_track_peak_t* out);

#ifdef __cplusplus
}
#endif
#endif
