/* uchirp_iir.h -- C-ABI of libuchirp_iir.so: the recursive filter bank of the chirp modem (biquad cascades over many rows).
 *
 * Every other stage of the chain is a finite sum or a 2048-point transform.  uc_iir_run is the recursive filter: n_rows
 * output rows, each one input row (float or DFSDM words) through a cascade of 1 .. 8 second-order sections in float32 -- the
 * Butterworth low-pass that the reference's lpf() runs through lfilter, a band-pass for 16 .. 19 kHz in front of the
 * correlators, a DC blocker behind the DFSDM, a microphone's own response, or one microphone through k band filters in one
 * call.  The state of every row lives in memory the caller owns, so a stream is filtered block by block.
 *
 * The library stands alone: it needs no symbol of the other libraries.  There is no CPU path behind uc_iir_run:
 * uc_iir_create fails without a GPU.  uc_iir_filter_row is pure host arithmetic and works anywhere.
 *
 * DEFINITION  (uchirp/iir.py holds it in numpy float32: `emulate32`)
 *
 * A filter is a cascade of n_sections sections, 1 .. 8.  A section is five floats b0 b1 b2 a1 a2 (a0 = 1) and carries two
 * floats of state per row, z1 and z2 (direct form II transposed).  A row's state is UC_IIR_STATE_WORDS = 16 floats: z1, z2 of
 * section 0, z1, z2 of section 1, ... of section 7.  All zeros is a filter at rest.  The words of sections that do not exist
 * are neither read nor changed.
 *
 * The input sample:
 *   UC_IIR_DTYPE_F32   the float as it is; a value that is not finite (NaN, +-Inf) reads as +0.
 *   UC_IIR_DTYPE_I32   (DFSDM words) (float)(word >> 8), arithmetic shift: the 24-bit value, exact.
 *
 * For sample u of a row the sections run in order, s = 0 .. n_sections - 1.  Every operation is ONE correctly rounded float32
 * multiply, add or subtract (round to nearest even); nothing is fused and nothing is reassociated:
 *   o  = (b0 * u) + z1
 *   z1 = ((b1 * u) - (a1 * o)) + z2
 *   z2 = (b2 * u) - (a2 * o)
 *   u  = o                               -> the next section; the last o is the output sample (a float)
 * Denormals are kept: they are not flushed on input, in the state or on output.
 *
 * The section count is part of the definition: a cascade padded with the identity section (1 0 0 0 0) gives +0 where the
 * shorter one gives -0.
 *
 * An output sample depends on its row's samples, its state and its coefficient set only, never on the grid, the other rows,
 * alignment, or how the row is cut into calls.  So uc_iir_run, uc_iir_filter_row and `emulate32` give the same bits.
 *
 * COEFFICIENT SETS AND FILTER BANKS
 *
 * An object holds up to UC_IIR_MAX_SETS sets of the same section count (uc_iir_set_sections).  Output row r reads input row
 * row_map[r] (NULL: r) through set set_index[r] (NULL: set 0).  One microphone through k band filters is one call with
 * n_in_rows = 1, n_rows = k, row_map all 0 and set_index 0 .. k - 1.
 *
 * OUT OF SCOPE: the mixer in front of a low-pass (the caller multiplies); decimation (uc_rate_convert does it); zero-phase
 * (forward-backward) filtering; more than 8 sections; coefficients that change from sample to sample; capture into a graph;
 * a check of stability: an unstable set is the caller's, and its infinities and NaNs are what IEEE arithmetic makes of it.
 */
#ifndef UCHIRP_IIR_H
#define UCHIRP_IIR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UC_IIR_ABI_VERSION 1

#define UC_IIR_DTYPE_I32 0 /* DFSDM words: the 24-bit value in bits 31:8 */
#define UC_IIR_DTYPE_F32 1

#define UC_IIR_MAX_SECTIONS 8
#define UC_IIR_MAX_SETS 256
#define UC_IIR_SECTION_WORDS 5 /* b0 b1 b2 a1 a2 */
#define UC_IIR_STATE_WORDS 16  /* z1, z2 of sections 0 .. 7 */

typedef struct uc_iir uc_iir;

int uc_iir_abi_version(void);
/* text of the calling thread's last error ("" if none) */
const char* uc_iir_last_error(void);

/* The definition in plain C for one row: n samples of `in` (float or int32 by `dtype`) through `sections` (n_sections x 5
 * floats) -> n floats; state[16] is read and brought up to date (the words of sections 0 .. n_sections - 1 only); needs no
 * GPU.  -EINVAL: a NULL pointer, n == 0, n_sections not in 1 .. 8, an unknown dtype, a coefficient that is not finite. */
int uc_iir_filter_row(const float* sections, int n_sections, const void* in, int dtype, size_t n, float state[16], float* out);

/* An object on one device, without coefficient sets.  -EINVAL: out is NULL; -ENODEV ("no CPU path") when no GPU is
 * visible. */
int uc_iir_create(int device, uc_iir** out);
/* Waits for the device, and with it for every call of the object on whatever stream it was given (a call that stages
 * nothing leaves no event to wait for), then frees it.  NULL is allowed. */
void uc_iir_destroy(uc_iir* iir);

/* Uploads n_sets coefficient sets of n_sections sections each (sections: n_sets x n_sections x 5 floats on the host); they
 * replace the object's sets.  Synchronous: it waits for the device before it writes, so no call in flight reads half a
 * table.  All or nothing: a refused call leaves the object's sets as they were.  -EINVAL: a NULL pointer, n_sets not in
 * 1 .. 256, n_sections not in 1 .. 8, a coefficient that is not finite. */
int uc_iir_set_sections(uc_iir* iir, const float* sections, size_t n_sets, int n_sections);

/* Filters n_samples samples of n_rows output rows.  in_dev (n_in_rows rows, float or int32 by in_dtype), state_dev (n_rows x
 * 16 floats, in and out: memory the caller owns) and out_dev (n_rows rows of floats) are device memory of the object's
 * device; input row i starts at in_dev + i * in_stride, output row r at out_dev + r * out_stride; strides are in elements,
 * 0 means n_samples.  row_map and set_index are host arrays of n_rows uint32 each, or NULL (row r, set 0); they are read
 * before the call returns.  Asynchronous on hip_stream (a hipStream_t, or NULL); the caller's current HIP device is
 * restored.  Any 4-byte alignment and any n_samples: tiles through LDS where pointers and strides put the rows on 16 bytes
 * and a wave's rows read their own input rows, dword or 16-byte accesses otherwise.  Every check and allocation comes before
 * the first launch: a refused call (negative errno) has enqueued nothing and leaves the object usable.  -EINVAL: a NULL
 * pointer (iir, in_dev, state_dev, out_dev); a zero count; n_rows or n_in_rows > 2^32 - 1; no sets uploaded; an unknown
 * dtype; a stride smaller than n_samples or larger than 2^40; a pointer that is not a multiple of 4; in_dev, state_dev or
 * out_dev not device memory of the object's device; row_map[r] >= n_in_rows; n_rows > n_in_rows without a row_map;
 * set_index[r] >= the number of sets; out_dev or state_dev overlapping in_dev or each other.  One thread at a time per
 * object; not capturable into a graph. */
int uc_iir_run(uc_iir* iir, const void* in_dev, int in_dtype, size_t n_in_rows, size_t in_stride, size_t n_rows, size_t n_samples,
               const uint32_t* row_map, const uint32_t* set_index, float* state_dev, float* out_dev, size_t out_stride, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
