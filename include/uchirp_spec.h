/* uchirp_spec.h -- C-ABI of libuchirp_spec.so: the spectrum analyser of the chirp modem (spectra and spectrograms of many
 * rows).
 *
 * The first thing the firmware does with a recording is to look at it: experiments/basic/Src/main.c:107-175 (fft())
 * multiplies a block by a Hann window, transforms it, takes the magnitude / sqrt(N), forces the bins below 1 kHz to 1,
 * prints 10 log10 of it and the frequency of the maximum; the notebooks draw spectrograms.  uc_spec_run is that for many
 * rows at once: every frame of every row -> its windowed 2048-point magnitude, power or level spectrum, any sub-range of
 * the bins, and each frame's largest stored value with its bin, in one launch.
 *
 * The library stands alone: it needs no symbol of the other nine libraries.  There is no CPU path: uc_spec_create fails
 * without a GPU.  uc_spec_plan and uc_spec_frames are pure host arithmetic and work anywhere.
 *
 * DEFINITION  (uchirp/spec.py holds it in float64: `model`; `emulate32` is an independent float32 evaluation)
 *
 * Input.  n_rows rows in device memory, UC_SPEC_DTYPE_F32 (float) or UC_SPEC_DTYPE_I32 (DFSDM words); every sample is cast
 * with (float).  Row m starts at in_dev + m * in_stride (elements) and holds n_in samples x_m[0 .. n_in - 1].  A sample
 * outside [0, n_in) reads as +0.0f.
 *
 * Frames.  Frame f = 0 .. n_frames - 1 of row m is, with P = 2048,
 *   u[i] = w[i] * x_m[first + f * hop + i]   for i < frame_len,       u[i] = +0.0f   for frame_len <= i < P
 * the product rounded to float.  first may be negative (centred frames) but lies above -frame_len and below n_in; hop >= 1
 * is any step, from overlap to gaps; frame_len is 1 .. 2048.  uc_spec_frames counts the frames f >= 0 whose first sample
 * first + f * hop lies below n_in, ceil((n_in - first) / hop): each of them overlaps the row; a call takes at most those.
 *
 * Window.  w is a table of frame_len floats that the object holds.  The default is the periodic Hann,
 * w[i] = (float)(0.5 - 0.5 cos(2 pi i / frame_len)) evaluated in double; uc_spec_set_window takes any host array (the
 * firmware's own table, say).
 *
 * Transform.  X[k] = sum_i u[i] exp(-2 pi j i k / P), k = 0 .. 1024, in float, by a 16 x 16 x 8 transform of (u, 0): each
 * frame has one transform of its own, as the real part of the complex input.  Two frames never share a transform (the
 * separation's error would scale with the other frame's norm), so a frame of zeros gives zeros exactly; that is part of the
 * definition.
 *
 * Values, in this order:
 *   1. v[k] = scale * sqrtf(fmaf(im, im, re * re)),  re + j im = X[k]
 *   2. v[k] = 1.0f for k < ac_bins (the firmware's AC coupling; 0 switches it off)
 *   3. UC_SPEC_MAG stores v[k];  UC_SPEC_POWER stores v[k] * v[k] (one rounding);
 *      UC_SPEC_DB stores db_mul * log10f(max(v[k], floor)).  db_mul = 10 is the firmware's (main.c:135: 10 log10 of a
 *      magnitude), 20 the usual one; floor > 0.
 * Bin 0 is |X[0]|.  DEVIATION: the firmware's bin 0 is hypot(X[0], X[1024]), because arm_rfft_fast_f32 packs the Nyquist
 * bin into the imaginary part of bin 0; in every capture the firmware printed, that bin lies under the AC coupling.
 *
 * Output.  Bins bin_first .. bin_first + n_bins - 1, a sub-range of 0 .. 1024, go to
 *   out_dev[(m * n_frames + f) * out_stride + (k - bin_first)]
 * and nothing else of out_dev is written.  If peaks_dev is not NULL, record m * n_frames + f of it is the frame's largest
 * STORED value and its bin; the lowest bin wins a tie (arm_max_f32, main.c:140).  A NaN is never the largest value; a frame
 * whose stored values are all NaN has { NaN, bin_first }.
 *
 * Non-finite samples.  One float sample x_m[q] that is NaN, +Inf or -Inf (integer words hold none):
 *   MUST      every frame f of row m with first + f * hop <= q < first + f * hop + frame_len has no finite X[k] -- also
 *             where w[i] is zero, as the periodic Hann's w[0] is: 0 * NaN is NaN.  UC_SPEC_MAG and UC_SPEC_POWER store a
 *             value that is not finite in every bin k >= ac_bins of such a frame (NaN for a NaN sample).  UC_SPEC_DB does
 *             NOT: max(v, floor) sends a NaN magnitude to the floor, so such a bin stores db_mul * log10f(floor), the
 *             level of silence, and +Inf where the magnitude is +Inf; a caller who must tell a dead microphone from a
 *             silent one asks for UC_SPEC_MAG or UC_SPEC_POWER.  The bins k < ac_bins store their constant (1.0f, 1.0f,
 *             db_mul * log10f(max(1.0f, floor))) in such a frame as in any other.
 *   MAY       nothing: a frame has a transform of its own.
 *   MUST NOT  every other frame of the row (a q that lies in a gap between frames touches none), every other row, their
 *             peak records, and every word of out_dev between the frames: bit for bit what the same call writes with a
 *             finite sample there.
 * Peak of such a frame: the rule above over what is stored.  For a NaN sample that is { NaN, bin_first } under UC_SPEC_MAG
 * and UC_SPEC_POWER if bin_first >= ac_bins, { 1.0f, bin_first } if the AC coupling covers bin_first; under UC_SPEC_DB the
 * finite { larger of the AC constant and the floor level, bin_first }.
 *
 * Invariance.  A frame's outputs depend on its samples, the window and the parameters only: never on the grid, the deal,
 * the other frames or rows of the call, or how a range of frames is cut into calls (first moved by whole hops).
 *
 * Error.  For UC_SPEC_MAG and a finite frame,
 *   |v_gpu[k] - v_exact[k]| <= UC_SPEC_ERROR_C * 2^-24 * |scale| * ||u||_2
 * where v_exact is the definition in exact arithmetic on the float samples and window.  The constant is measured, not
 * derived: four times the worst ratio an independent float32 evaluation of the same definition (numpy's float32 rfft of the
 * float32 product) reaches on the test inputs, rounded up.  UC_SPEC_POWER is fl(v * v) of the kernel's
 * own v bit for bit; UC_SPEC_DB lies within |db_mul| * UC_SPEC_LOG10_ERROR of db_mul * log10 of the kernel's own
 * max(v, floor) for 1e-8 <= max(v, floor) <= 1e8 (lambda is measured like C: DESIGN.md section 18).
 *
 * OUT OF SCOPE: transforms other than 2048 points; averaging frames (Welch); complex output; int16 input (uc_rate_convert
 * makes float); capture into a graph.
 */
#ifndef UCHIRP_SPEC_H
#define UCHIRP_SPEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UC_SPEC_ABI_VERSION 1

#define UC_SPEC_DTYPE_I32 0 /* DFSDM words */
#define UC_SPEC_DTYPE_F32 1

#define UC_SPEC_MAG 0
#define UC_SPEC_POWER 1
#define UC_SPEC_DB 2

#define UC_SPEC_POINTS 2048 /* P */
#define UC_SPEC_BINS 1025   /* bins 0 .. P / 2 */

#define UC_SPEC_ERROR_C 200           /* C of the error form */
#define UC_SPEC_LOG10_ERROR 5.0e-6f   /* lambda of the error form */

typedef struct uc_spec uc_spec;

/* what a call computes (56 bytes) */
typedef struct uc_spec_params {
  int64_t first;      /* row element of frame 0's first sample; -frame_len < first < n_in */
  uint64_t n_frames;  /* frames of every row; 0: all that uc_spec_frames counts */
  uint32_t frame_len; /* 1 .. 2048 */
  uint32_t hop;       /* >= 1 */
  uint32_t bin_first; /* bin_first + n_bins <= 1025 */
  uint32_t n_bins;    /* >= 1 */
  uint32_t ac_bins;   /* bins below it store as v = 1.0f; 0: none */
  int32_t kind;       /* UC_SPEC_MAG, UC_SPEC_POWER, UC_SPEC_DB */
  float scale;        /* finite */
  float floor;        /* > 0 and finite (read by UC_SPEC_DB) */
  float db_mul;       /* finite (read by UC_SPEC_DB) */
  uint32_t reserved;  /* 0 */
} uc_spec_params;

/* what uc_spec_plan makes of it (32 bytes) */
typedef struct uc_spec_info {
  uint64_t n_frames;   /* frames of every row */
  uint64_t out_stride; /* elements between two frames of out_dev (the given one, or n_bins) */
  uint64_t out_elems;  /* elements from the first one written to the last: (n_rows * n_frames - 1) * out_stride + n_bins */
  uint32_t bin_first;
  uint32_t n_bins;
} uc_spec_info;

/* one frame's largest stored value (8 bytes) */
typedef struct uc_spec_peak {
  float value;
  uint32_t bin;
} uc_spec_peak;

int uc_spec_abi_version(void);
/* text of the calling thread's last error ("" if none) */
const char* uc_spec_last_error(void);

/* The frames f >= 0 whose first sample first + f * hop lies below n_in; needs no GPU.  -EINVAL: n_in 0 or above 2^40,
 * frame_len not in 1 .. 2048, hop 0, first <= -frame_len or first >= n_in. */
int64_t uc_spec_frames(uint64_t n_in, int64_t first, uint32_t frame_len, uint32_t hop);

/* Checks what uc_spec_run checks of the numbers alone and reports the frames, the bins and the output elements; needs no
 * GPU.  -EINVAL: params or info is NULL; n_rows 0 or above 2^32 - 1; what uc_spec_frames refuses; n_frames above its
 * count; a bin range that is empty or leaves 0 .. 1024; out_stride < n_bins (unless 0: n_bins); an unknown kind; scale or
 * db_mul not finite; floor not finite or <= 0; reserved not 0; n_rows * n_frames above 2^40 or an output above 2^58
 * elements.  *info is written on success only. */
int uc_spec_plan(const uc_spec_params* params, size_t n_rows, size_t n_in, size_t out_stride, uc_spec_info* info);

/* An object on one device; its window is the periodic Hann of 2048 values.  -ENODEV ("no CPU path") when no GPU is visible. */
int uc_spec_create(int device, uc_spec** out);
/* Waits for the device, and with it for every call of the object on whatever stream it was given (a call that stages
 * nothing leaves no event to wait for), then frees it.  NULL is allowed. */
void uc_spec_destroy(uc_spec* spec);

/* The object's window: len floats of a host array, or -- window NULL -- the periodic Hann of len values.  Synchronous: it
 * waits for the device, and with it for every call of the object on whatever stream it was given, then copies.
 * -EINVAL: spec NULL, len not in 1 .. 2048, a value that is not finite. */
int uc_spec_set_window(uc_spec* spec, const float* window, size_t len);

/* The spectra of the definition for n_frames frames of each of n_rows rows.  in_dev, out_dev and peaks_dev (or NULL) are
 * device memory of the object's device; strides are in elements, 0 means the count (n_in, n_bins).  Asynchronous on
 * hip_stream (a hipStream_t, or NULL); the caller's current HIP device is restored.  The call reads no host array but
 * *params, which it has read when it returns.  Every argument is checked before the only launch: a refused call (negative
 * errno) has enqueued nothing and leaves the object usable.  -EINVAL: what uc_spec_plan refuses; in_stride < n_in; an
 * unknown dtype; a NULL pointer; params->frame_len that is not the length of the object's window; memory that is not the
 * object's device's; out_dev, peaks_dev or in_dev overlapping one another.  One thread at a time per object; not capturable
 * into a graph. */
int uc_spec_run(uc_spec* spec, const void* in_dev, int in_dtype, size_t n_rows, size_t n_in, size_t in_stride,
                const uc_spec_params* params, float* out_dev, size_t out_stride, uc_spec_peak* peaks_dev, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
