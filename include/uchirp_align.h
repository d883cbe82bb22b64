/* uchirp_align.h -- C-ABI of libuchirp_align.so: the delay estimator of the chirp modem (cross-correlation of array
 * microphones with a reference microphone, and the crest rule that turns a correlation into a fractional delay).
 *
 * uc_array_combine (uchirp_array.h) needs every microphone's fractional delay.  For a buffer the scene renderer made
 * they come from the scene; a recording has none.  This library estimates them from the samples: uc_align_correlate
 * correlates pairs of rows over a window of lags on the GPU, uc_align_peak reads the delay off one correlation on the
 * host.
 *
 * The library stands alone: it needs no symbol of libuchirp.so, libuchirp_link.so, libuchirp_scene.so or
 * libuchirp_array.so.  There is no CPU path: uc_align_create fails without a GPU.  uc_align_peak is pure host arithmetic
 * and works anywhere.
 *
 * DEFINITION OF THE CORRELATION
 *
 * Input.  n_mics rows in device memory, UC_ALIGN_DTYPE_F32 (float) or UC_ALIGN_DTYPE_I32 (DFSDM words, each cast with
 * (float) as the receivers do).  Row m starts at in_dev + m * in_stride (elements) and holds n_in samples.  x_m[j] is
 * sample j of row m after the cast; a sample of the MICROPHONE row outside [0, n_in) reads as +0.0f (the reference row is
 * only read inside [first, first + n), which lies inside the row).
 *
 * Pair.  { ref, mic }: two rows (they may be the same row).  With L = max_lag, for l = -L .. L
 *   r_p[l] = sum over j = first .. first + n - 1 of  x_ref[j] * x_mic[j + l]
 * is stored as a double at corr_dev[p * corr_stride + (l + L)].  A positive lag of the crest means that the microphone
 * hears the sound LATER than the reference: it is the delay_samples of uc_array_tap against the reference.
 *
 * Summation order.  Let i = j - first.  The range is cut into segments of UC_ALIGN_SEGMENT = 4096 samples counted from
 * first: segment s holds i = 4096 s .. min(4096 s + 4095, n - 1); the last one may be short.  Within a segment let
 * i' = i - 4096 s; sample i' belongs to CHAIN (i' mod 256) div 4, one of 64.  For one lag,
 *   - every chain starts at +0.0f and takes its samples in ascending i':  a = fmaf(x_ref[j], x_mic[j + l], a)
 *     (at most 64 fused multiply-adds; in a short segment a chain may be shorter or empty);
 *   - the 64 chain sums c[0 .. 63] are added in float as a tree, each addition rounded once:
 *     c[k] = c[k] + c[k + h] for k < h, for h = 32, 16, 8, 4, 2, 1 in that order; the segment's sum is c[0].
 * The longest path from a product to the segment's sum has UC_ALIGN_ROUNDINGS = K = 70 float roundings (64 in the chain,
 * 6 in the tree).  The segment sums are converted to double and added in double, starting from 0.0, in ascending
 * segment order.  So |r_p[l] - exact| <= K * 2^-24 * sum_j |x_ref[j] * x_mic[j + l]| to first order, and a result
 * depends on the inputs, the pair, first, n and L only: never on the grid, on which wave handled which segment, or on the
 * other pairs of the call.
 *
 * Non-finite samples.  One float sample x_m[q] that is NaN, +Inf or -Inf (integer words hold none):
 *   MUST      r_p[l] is not finite wherever its sum has a term with x_m[q]: for every l if m is the pair's reference row and
 *             first <= q < first + n (also where the other factor is a microphone sample outside the row, +0.0f); for the
 *             lags with first <= q - l < first + n if m is the pair's microphone row.
 *   MAY       if m is the pair's microphone row, also the lags with first + n <= q - l < first + n_up, where n_up is n with
 *             its last segment rounded up to a multiple of 256 samples (n_up - n <= 255): a segment is walked in passes
 *             of 256 reference samples, and in the last, partial pass the lanes behind the reference's end hold +0.0f and
 *             still multiply the microphone samples opposite them (0 * NaN is NaN).  So the last microphone sample that
 *             can reach a sum is first + n_up + L - 1, and it reaches lag +L alone.  Such a value is either bit for bit the
 *             clean call's or not finite (this implementation: not finite), never another finite number.
 *   MUST NOT  everything else the call writes -- the other lags of the pair, all other pairs, and every word of corr_dev
 *             between the rows -- is bit for bit what the same call writes with a finite sample there.
 * uc_align_peak refuses a correlation with a value that is not finite (-EINVAL): it is the host's detector.
 *
 * DEFINITION OF THE PEAK (uc_align_peak; double arithmetic on the host)
 *
 * The chirp band is narrow (16 - 19 kHz at 78 125 samples/s), so a correlation is a carrier of period ~4.5 samples under
 * an envelope ~26 samples wide, and the crest next to the true one is only ~5 % lower: the largest SAMPLE of r is the
 * wrong crest in nearly half of all pairs at any SNR, because the sample grid favours whichever crest falls nearest a
 * sample.  The rule fits a sinusoid through three points at every local maximum and takes the crest whose FITTED height
 * is greatest.  With r[k], k = 0 .. 2L, the values for l = k - L:
 *   a candidate is every k in 1 .. 2L - 1 with r[k] > 0, r[k] >= r[k-1] and r[k] > r[k+1];
 *   c = (r[k-1] + r[k+1]) / (2 r[k]);
 *   if -1 < c < 1:  w = acos(c),  q = (r[k+1] - r[k-1]) / (2 sin w),  height = hypot(r[k], q),  d = atan2(q, r[k]) / w
 *   otherwise       height = r[k],  d = 0;
 *   the estimate is the candidate of greatest height, the first one on a tie.
 * (Three samples A cos(w (k + t - k0)), t = -1, 0, 1, give exactly c = cos w, q = A sin(w (k0 - k)), height = A,
 * d = k0 - k.)
 *
 * OUT OF SCOPE: PHAT or other spectral weightings; FFT-based correlation for lag ranges beyond UC_ALIGN_MAX_LAG; tracking
 * delays over time; per-microphone clock offsets (an array shares one clock); adaptive weights; capture into a graph;
 * resolving whole-cycle ambiguity at low SNR beyond reporting runner_up (at -12 dB about half of the pairs land whole
 * carrier cycles off; delay-and-sum beams of eight microphones steered that way still decoded).
 * Weights on the chirps' band, which keep the crest on its cycle at low SNR: uchirp_wcorr.h.
 */
#ifndef UCHIRP_ALIGN_H
#define UCHIRP_ALIGN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UC_ALIGN_ABI_VERSION 1

#define UC_ALIGN_DTYPE_I32 0 /* DFSDM words */
#define UC_ALIGN_DTYPE_F32 1

#define UC_ALIGN_MAX_LAG 64   /* L = max_lag is 1 .. 64 */
#define UC_ALIGN_SEGMENT 4096 /* samples of one float sum */
#define UC_ALIGN_ROUNDINGS 70 /* K: float roundings on the longest path from a product to a segment's sum */

#define UC_ALIGN_NO_PEAK 1u /* flags: no candidate; delay_samples, height, lag and runner_up are 0 */
#define UC_ALIGN_AT_EDGE 2u /* flags: the largest sample of r lies at index 0 or 2L: the true crest may lie outside */

typedef struct uc_align uc_align;

/* one pair of rows (8 bytes) */
typedef struct uc_align_pair {
  uint32_t ref; /* row of the reference microphone (< n_mics) */
  uint32_t mic; /* row of the microphone (< n_mics) */
} uc_align_pair;

/* what uc_align_peak reads off one correlation (32 bytes) */
typedef struct uc_align_peak_t {
  double delay_samples; /* k - L + d of the chosen candidate */
  double height;        /* its fitted height */
  double runner_up;     /* second-greatest candidate height / height, 0 with one candidate: near 1 means that a whole
                           carrier cycle more or less fits almost as well */
  int32_t lag;          /* k - L */
  uint32_t flags;       /* UC_ALIGN_NO_PEAK | UC_ALIGN_AT_EDGE */
} uc_align_peak_t;

int uc_align_abi_version(void);
/* text of the calling thread's last error ("" if none) */
const char* uc_align_last_error(void);
/* -ENODEV ("no CPU path") when no GPU is visible */
int uc_align_create(int device, uc_align** out);
/* Waits for every call of the object still in flight, on whatever streams they were given (each call is ordered behind the
 * call two before it, so the events of the last two cover all), then frees it.  NULL is allowed. */
void uc_align_destroy(uc_align* align);

/* The correlations of the definition for n_pairs pairs.  pairs is a HOST array: it is copied, with the records derived
 * from it, into one of two pinned staging buffers of the object, used in turn, before the call returns (the caller may
 * reuse it at once), and from there to the device on hip_stream.  in_dev and corr_dev are device memory of the object's
 * device; strides are in elements (of the input's type, of double), 0 means the count (n_in, 2 max_lag + 1).  Only the
 * 2 max_lag + 1 doubles of every row of corr_dev are written.  Asynchronous on hip_stream (a hipStream_t, or NULL); the
 * caller's current HIP device is restored.  Every argument is checked and every buffer is sized before anything is
 * enqueued: a refused call (negative errno) has enqueued nothing and leaves the object usable.  -EINVAL: a pair's ref or
 * mic >= n_mics; first + n > n_in; max_lag not in 1 .. UC_ALIGN_MAX_LAG; corr_stride < 2 max_lag + 1 (unless 0);
 * in_stride < n_in (unless 0); a zero count (n_mics, n_in, n_pairs, n); an unknown dtype; a NULL array; in_dev or
 * corr_dev not device memory of the object's device; corr_dev overlapping in_dev.  One thread at a time per object; not
 * capturable into a graph. */
int uc_align_correlate(uc_align* align, const void* in_dev, int in_dtype, size_t n_mics, size_t n_in, size_t in_stride,
                       const uc_align_pair* pairs, size_t n_pairs, size_t first, size_t n, uint32_t max_lag, double* corr_dev,
                       size_t corr_stride, void* hip_stream);

/* The peak of the definition over corr[0 .. 2 max_lag] (HOST memory); needs no GPU.  -EINVAL: a NULL pointer, max_lag
 * not in 1 .. UC_ALIGN_MAX_LAG, a value that is not finite. */
int uc_align_peak(const double* corr, uint32_t max_lag, uc_align_peak_t* out);

#ifdef __cplusplus
}
#endif
#endif
