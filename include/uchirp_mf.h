/* uchirp_mf.h -- C-ABI of libuchirp_mf.so: the pulse compressor of the chirp modem (many rows, real or complex, filtered
 * with known pulses by overlap-save on 2048-point transforms, and a small arrival record per segment, so that a caller who
 * wants to know WHEN a pulse arrived need not store an envelope).
 *
 * It is the reference's "Compress chirp in time domain" experiment (simulation/ChirpSimulation.ipynb,
 * sg.lfilter(matched_filter, 1, receive_buf) and its ifft(fft * fft) twin) for many rows and several templates per call,
 * and the step between uc_ddc_run (uchirp_ddc.h), whose UC_DDC_OUT_IQ rows it reads as they are, and any ranging,
 * multipath profiling or symbol timing on an array.
 *
 * The library stands alone: it needs no symbol of the other libraries.  There is no CPU path: uc_mf_create fails
 * without a GPU.  uc_mf_plan, uc_mf_spectrum, uc_mf_select and uc_mf_arrival are pure host arithmetic and work anywhere.
 *
 * DEFINITION
 *
 * Input.  n_rows rows in device memory: UC_MF_DTYPE_F32 (float), UC_MF_DTYPE_I32 (DFSDM words, each cast with (float)) or
 * UC_MF_DTYPE_C32 (interleaved float pairs I, Q: what UC_DDC_OUT_IQ writes).  Row r starts at in_dev + r * in_stride
 * (elements: words, or pairs) and holds n_in elements.  x_r[j] is element j as a complex number, with imaginary part +0
 * for the real types; outside [0, n_in) a row reads +0.  What a float that is not finite does: "Non-finite samples" below.
 *
 * Templates.  uc_mf_set_templates(mf, taps, n_sets, n_taps): n_sets = 1 .. UC_MF_MAX_SETS sets of T = n_taps =
 * 1 .. UC_MF_MAX_TAPS complex taps h_s[t], a host array of n_sets * n_taps float pairs.  With P = UC_MF_POINTS = 2048,
 *   H_s[k] = the float32 rounding of (sum over t of h_s[t] * exp(-2 pi i k t / P)) / P,   k = 0 .. P - 1,
 * evaluated in double on the host: uc_mf_spectrum is that computation.
 *
 * Output.  y[q] = sum over k < T of h[k] * x[q - k]: lfilter(h, 1, x).  A matched filter is the caller passing the
 * reversed conjugate of the pulse.  q is an ABSOLUTE index: element j of a row is sample pos0 + j, pos0 a uint64_t.
 *
 * Segments.  S = P - T - 1 is the hop.  Segment k covers the outputs k S .. k S + S - 1 of the absolute axis.  Its
 * window is a_k[t] = x[k S - T + t], t = 0 .. P - 1, and it is evaluated in float as
 *   inverse transform(transform(a_k) * H)
 * (the inverse transform is not normalised: H holds the 1 / P).  Positions t = T - 1 .. P - 1 of the result are
 * y[k S - 1] .. y[k S + S]: the segment's S outputs and one neighbour on each side; nothing there wraps.  A call
 * produces the outputs pos0 + first .. pos0 + first + n - 1 (first + n <= n_in): those of the segments
 * first_segment .. first_segment + n_segments - 1 of uc_mf_plan, the first and last possibly in part.
 * A caller who wants denser records pads the template with zero taps: S shrinks with T.
 *
 * Power.  e[q] = fmaf(re, re, im * im) of y[q], the product im * im rounded first.
 *
 * Record.  One per (job, segment), uc_mf_record, 80 bytes.  A CANDIDATE is an output q of the segment inside the call's
 * range with e[q] >= e[q - 1] and e[q] > e[q + 1]; the neighbours are always the transform's own values, also where they
 * lie outside the range or the segment.  The record keeps the UC_MF_CANDIDATES = 4 candidates of greatest e, the lower q
 * first on a tie, in that order, each as { offset = q - k S, e[q - 1], e[q], e[q + 1] }; unused slots are zero.  n_cand is
 * the number of candidates of the segment (it may exceed 4), count the number of the segment's outputs in range, sum
 * their e added in float -- in an order that is the kernel's own, but never depends on the grid.  uc_mf_select is the
 * same rule in plain C over an array of e (its sum is added in ascending order).  uc_mf_arrival fits the parabola
 * through the SQUARE ROOTS of a candidate's three values, in double: with a, b, c the roots and d = a - 2 b + c, the
 * vertex lies at delta = (a - c) / (2 d) with height b - (a - c) delta / 4 if d < 0; otherwise delta = 0 and the
 * height is b.  *offset = cand->offset + delta.
 *
 * Jobs.  uc_mf_job { row, set }: output row i and record row i belong to job i.  One microphone through k templates is
 * k jobs (up and down chirps, or several transmitters' pulses).
 *
 * Formats.  UC_MF_OUT_COMPLEX float pairs (re, im); UC_MF_OUT_REAL re; UC_MF_OUT_POWER e; UC_MF_OUT_MAG the correctly
 * rounded sqrtf(e).  Output row i starts at out_dev + i * out_stride (elements of the format) and holds the call's n
 * outputs; record row i starts at records_dev + i * n_segments.  out_dev and records_dev are each nullable.
 *
 * Invariance.  A stored value or a record depends on the segment's window as it reads in the call, the template and q:
 * never on the grid, on the other jobs or their order, or on the staging slot.  A segment that lies wholly in the range
 * of two calls, with its window inside the row in both, has the same bits in both: that is what a live caller who keeps
 * T samples of history gets.
 *
 * Non-finite samples.  One float of row r -- element q, or the real or the imaginary part of it alone -- that is NaN,
 * +Inf or -Inf (integer words hold none), in every job { r, set }:
 *   MUST      y of row element e is not finite in every format (the pair, its real part, its power, its magnitude) wherever its
 *             sum has a term with x[q]: e - T + 1 <= q <= e, for the e inside the call's range.
 *   MAY       all other outputs of a segment k whose WINDOW holds q, a_k = row elements k S - pos0 - T .. k S - pos0 + S,
 *             cut at the row and not at the call's first + n: a segment comes out of one inverse transform (this
 *             implementation: they are all not finite).  The window is one element wider on each side than the sums of
 *             the segment's outputs reach (they read k S - pos0 - T + 1 .. k S - pos0 + S - 1; the two neighbours the
 *             record looks at read the rest), and it reaches behind first + n: a sample no output of the call reads can
 *             take a whole segment with it.  Such a value is either bit for bit the clean call's or not finite, never
 *             another finite number.
 *   MUST NOT  every segment whose window does not hold q, every other row's jobs, their records, and every word of out_dev
 *             between the rows: bit for bit what the same call writes with a finite sample there.
 * Record of a segment with a power that is not finite: n_cand = 0, four zero slots, count as usual, and a sum that is not
 * finite (no comparison with a NaN holds, and +Inf is not greater than +Inf).  !isfinite(sum) is the caller's test: such a
 * segment never reports a candidate.  A MAY segment's record is either that or bit for bit the clean one.
 *
 * Error.  With a_k the window and h the template,
 *   |y[q] - exact| <= UC_MF_ERROR_C * 2^-24 * ||a_k||_2 * ||h||_2.
 * The constant is measured, not derived: four times the worst ratio an independent float32 evaluation of the same
 * definition reaches on the test inputs, rounded up.
 *
 * OUT OF SCOPE: templates beyond UC_MF_MAX_TAPS or other transform lengths; a fused mixer (uc_ddc_run); detection rules
 * beyond a ratio to the segment's mean; capture into a graph.
 */
#ifndef UCHIRP_MF_H
#define UCHIRP_MF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UC_MF_ABI_VERSION 1

#define UC_MF_DTYPE_I32 0 /* DFSDM words */
#define UC_MF_DTYPE_F32 1
#define UC_MF_DTYPE_C32 2 /* float pairs I, Q */

#define UC_MF_OUT_COMPLEX 0
#define UC_MF_OUT_REAL 1
#define UC_MF_OUT_POWER 2
#define UC_MF_OUT_MAG 3

#define UC_MF_POINTS 2048   /* P: length of the transforms */
#define UC_MF_MAX_TAPS 1664 /* T = n_taps is 1 .. 1664; the hop S = P - T - 1 is 2046 .. 383 */
#define UC_MF_MAX_SETS 256
#define UC_MF_CANDIDATES 4
#define UC_MF_ERROR_C 9 /* C of the error form */

typedef struct uc_mf uc_mf;

/* one job (8 bytes) */
typedef struct uc_mf_job {
  uint32_t row; /* < n_rows */
  uint32_t set; /* < n_sets of the last uc_mf_set_templates */
} uc_mf_job;

/* one candidate (16 bytes) */
typedef struct uc_mf_candidate {
  uint32_t offset; /* q - k S: 0 .. S - 1 */
  float left;      /* e[q - 1] */
  float peak;      /* e[q] */
  float right;     /* e[q + 1] */
} uc_mf_candidate;

/* what a call leaves of one segment of one job (80 bytes) */
typedef struct uc_mf_record {
  uc_mf_candidate cand[UC_MF_CANDIDATES]; /* by falling e, the lower q first on a tie; unused slots are zero */
  float sum;                              /* of e over the segment's outputs in range */
  uint32_t count;                         /* the segment's outputs in range */
  uint32_t n_cand;                        /* its candidates (may exceed UC_MF_CANDIDATES) */
  uint32_t reserved;                      /* 0 */
} uc_mf_record;

int uc_mf_abi_version(void);
/* text of the calling thread's last error ("" if none) */
const char* uc_mf_last_error(void);
/* -ENODEV ("no CPU path") when no GPU is visible */
int uc_mf_create(int device, uc_mf** out);
/* Waits for every call of the object still in flight, on whatever streams they were given (each call is ordered behind the
 * call two before it, so the events of the last two cover all), then frees it.  NULL is allowed. */
void uc_mf_destroy(uc_mf* mf);

/* The hop and the segments of a call; needs no GPU.  *hop = S; the call's outputs are those of the segments
 * *first_segment .. *first_segment + *n_segments - 1.  -EINVAL: n_taps not in 1 .. UC_MF_MAX_TAPS, n = 0, a NULL
 * pointer, pos0 + first + n beyond 2^64 - 1. */
int uc_mf_plan(uint32_t n_taps, uint64_t pos0, size_t first, size_t n, uint32_t* hop, uint64_t* first_segment, uint64_t* n_segments);

/* H of the definition for one set: taps holds n_taps float pairs, spectrum receives UC_MF_POINTS float pairs (HOST
 * memory); needs no GPU.  -EINVAL: a NULL pointer, n_taps not in 1 .. UC_MF_MAX_TAPS, a tap that is not finite. */
int uc_mf_spectrum(const float* taps, uint32_t n_taps, float* spectrum);

/* The record of the definition over e[0 .. hop + 1] (HOST memory), e[1 + u] the power of the segment's output u, e[0]
 * and e[hop + 1] the neighbours' (outputs -1 and S); the outputs lo .. hi - 1 are in range; needs no GPU.  sum is added
 * in ascending order.  -EINVAL: a NULL pointer, hop not in 1 .. UC_MF_POINTS - 2, lo >= hi or hi > hop. */
int uc_mf_select(const float* e, uint32_t hop, uint32_t lo, uint32_t hi, uc_mf_record* out);

/* The arrival of the definition; needs no GPU.  -EINVAL: a NULL pointer, a negative or non-finite value. */
int uc_mf_arrival(const uc_mf_candidate* cand, double* offset, double* height);

/* The object's templates (see the definition).  taps is a HOST array.  Synchronous: it waits for the object's calls in
 * flight on whatever streams they were given (the events of the last two calls: each call is ordered behind the call two
 * before it), and returns with the spectra on the device.  All or nothing: a refused call leaves the former templates in
 * place.  -EINVAL: a NULL pointer, n_sets not in 1 .. UC_MF_MAX_SETS, n_taps not in 1 .. UC_MF_MAX_TAPS, a tap that is
 * not finite. */
int uc_mf_set_templates(uc_mf* mf, const float* taps, uint32_t n_sets, uint32_t n_taps);

/* The outputs pos0 + first .. pos0 + first + n - 1 of n_jobs jobs and / or their records.  jobs is a HOST array: it is
 * copied, with the records derived from it, into one of two pinned staging buffers of the object, used in turn, before
 * the call returns (the caller may reuse it at once), and from there to the device on hip_stream.  in_dev, out_dev and
 * records_dev are device memory of the object's device; strides are in elements (of the input's type, of the output's
 * format), 0 means the count (n_in, n).  Only the n outputs of every row of out_dev are written, and
 * n_jobs * n_segments records.  Asynchronous on hip_stream (a hipStream_t, or NULL); the caller's current HIP device is
 * restored.  Every argument is checked and every buffer is sized before anything is enqueued: a refused call (negative
 * errno) has enqueued nothing and leaves the object usable.  -EINVAL: no templates set; a job's row >= n_rows or set >=
 * n_sets; first + n > n_in; pos0 + n_in beyond 2^64 - 1; out_stride < n (unless 0); in_stride < n_in (unless 0); a zero
 * count (n_rows, n_in, n_jobs, n); an unknown dtype or format; a NULL array; out_dev and records_dev both NULL; in_dev,
 * out_dev or records_dev not device memory of the object's device; out_dev or records_dev overlapping in_dev or each
 * other.  One thread at a time per object; not capturable into a graph. */
int uc_mf_run(uc_mf* mf, const void* in_dev, int in_dtype, size_t n_rows, size_t n_in, size_t in_stride, const uc_mf_job* jobs,
              size_t n_jobs, uint64_t pos0, size_t first, size_t n, void* out_dev, int out_format, size_t out_stride,
              uc_mf_record* records_dev, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
