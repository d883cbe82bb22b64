/* uchirp_ddc.h -- C-ABI of libuchirp_ddc.so: the down-converter of the chirp modem (mix, FIR and decimate many rows to I/Q).
 *
 * The reference's iq_demodulation() (experiments/iq_modulation/Src/iq_modem.c) multiplies a block by a carrier's cosine and
 * sine and runs both products through a 27-tap FIR whose state persists from block to block; its notebook does the same on
 * recorded rows.  uc_ddc_run is that stage for many rows at once: n_rows output rows, each one input row (float or DFSDM
 * words) times the carrier of a 32-bit phase accumulator, through a FIR of 1 .. 128 taps, decimated by 1 .. 64, as
 * interleaved I, Q pairs or as the I chain alone (with step 0 and phase 0: a plain real FIR bank).  The history of every
 * input row lives in memory the caller owns, so a stream is converted block by block; with row_map, set_index, step and
 * phase0 one microphone is converted at k carriers in one call.
 *
 * The library stands alone: it needs no symbol of the other libraries.  There is no CPU path behind uc_ddc_run:
 * uc_ddc_create fails without a GPU.  uc_ddc_filter_row, uc_ddc_outputs and uc_ddc_carrier_tables are pure host arithmetic
 * and work anywhere.
 *
 * DEFINITION  (uchirp/ddc.py holds it in numpy float32: `emulate32`; uc_ddc_filter_row holds it in plain C)
 *
 * The input sample x:
 *   UC_DDC_DTYPE_F32   the float as it is; a value that is not finite (NaN, +-Inf) reads as +0.
 *   UC_DDC_DTYPE_I32   (DFSDM words) (float)(word >> 8), arithmetic shift: the 24-bit value, exact.
 * Denormals are kept everywhere: on input, in the products, in the sums and on output.
 *
 * The carrier of output row r is a 32-bit phase accumulator with step[r] and phase0[r] (uint32).  The sample with the
 * absolute index n (uint64; the indices in front of 0 wrap, which is the same modulo 2^32) has the phase
 *   phi = (phase0 + step * n) mod 2^32,
 * whatever the cut of the row into calls.  The top 10 bits of phi index the coarse table, 1024 pairs (cc, sc) = (cos, sin)
 * of 2 pi i / 2^10; the next 10 bits index the fine table, 1024 pairs (cf, sf) of 2 pi f / 2^20; the low 12 bits are
 * dropped.  Then, every operation ONE correctly rounded float32 operation and nothing fused,
 *   c = (cc * cf) - (sc * sf)            s = (sc * cf) + (cc * sf)
 * The tables are part of the definition: the library computes them in double and rounds them to float;
 * uc_ddc_carrier_tables hands them out.  Properties (tests/test_ddc_cpu.py measures them): (c, s) lies within 1.1e-7 of the
 * cosine and sine of the truncated phase and within 6.0e-6 (2 pi / 2^20) of those of the full phase; a carrier on a bin
 * of the receivers' 2048-point transform, or of one of 65 536 points, has no spur above -165 dBc (-161 dBc at 4096 and 8192
 * points).  With step 0 and phase0 0 the carrier is exactly (1, 0).
 *
 * The mixer: mi = x * c, mq = x * s, one rounding each (I from the cosine, Q from the sine, as iq_modem.c); a negative
 * frequency is the two's-complement step.
 *
 * The filter: a set of n_taps taps h, 1 .. UC_DDC_MAX_TAPS, and a decimation D, 1 .. UC_DDC_MAX_DECIM, one value per object.
 * The output with the absolute index p belongs to the sample n = p * D:
 *   acc = +0;  for k = 0 .. n_taps - 1:  acc = fmaf(h[k], m[n - k], acc)
 * one chain over mi for I and one over mq for Q, in this order of k.  n_taps is part of the definition: a set padded with
 * zero taps gives +0 where the shorter one gives -0.
 *
 * Output formats: UC_DDC_OUT_IQ, interleaved float pairs I, Q; UC_DDC_OUT_I, the I chain alone (Q is not computed).
 *
 * Positions: a call carries `first`, the absolute index of in[0], shared by all rows, and produces the outputs p with
 * first <= p * D <= first + n_samples - 1; the first of them lands at element 0 of the output row.  uc_ddc_outputs tells which
 * they are.  There may be none: the call then only brings the state up to date.
 *
 * The state: UC_DDC_STATE_WORDS = 128 floats per INPUT row, the 128 converted input samples in front of `first`, oldest first
 * (unmixed: the carrier of a past sample is recomputed from its index, with the same bits, so rows that share an input row
 * share its state).  All zeros is a filter at rest (arm_fir_init_f32's zeroed state at first = 0).  A call of fewer than 128
 * samples shifts the state.
 *
 * An output value depends on its row's samples, state, taps, step, phase and position only, never on the grid, the other
 * rows, alignment, or how the row is cut into calls.  So uc_ddc_run, uc_ddc_filter_row and `emulate32` give the same bits.
 *
 * BANKS
 *
 * An object holds up to UC_DDC_MAX_SETS tap sets of one n_taps (uc_ddc_set_taps).  Output row r reads input row row_map[r]
 * (NULL: r) through set set_index[r] (NULL: set 0) with step[r] (NULL: 0) and phase0[r] (NULL: 0).  One microphone against k
 * carriers is one call with n_in_rows = 1, n_rows = k and row_map all 0.
 *
 * OUT OF SCOPE: taps that change from sample to sample; complex input; more than 128 taps or a decimation above 64;
 * interpolation (uc_rate_convert does it); capture into a graph; a transform-domain (overlap-save) form for long filters: it
 * would change the bits.
 */
#ifndef UCHIRP_DDC_H
#define UCHIRP_DDC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UC_DDC_ABI_VERSION 1

#define UC_DDC_DTYPE_I32 0 /* DFSDM words: the 24-bit value in bits 31:8 */
#define UC_DDC_DTYPE_F32 1

#define UC_DDC_OUT_IQ 0 /* interleaved float pairs I, Q */
#define UC_DDC_OUT_I 1  /* the I chain alone */

#define UC_DDC_MAX_TAPS 128
#define UC_DDC_MAX_DECIM 64
#define UC_DDC_MAX_SETS 256
#define UC_DDC_STATE_WORDS 128 /* the converted input samples in front of `first`, oldest first */
#define UC_DDC_TABLE_WORDS 2048 /* 1024 (cos, sin) pairs */

typedef struct uc_ddc uc_ddc;

int uc_ddc_abi_version(void);
/* text of the calling thread's last error ("" if none) */
const char* uc_ddc_last_error(void);

/* The carrier's tables: coarse[2 i], coarse[2 i + 1] = cos, sin of 2 pi i / 2^10 and fine[2 f], fine[2 f + 1] = cos, sin of
 * 2 pi f / 2^20, computed in double and rounded to float.  -EINVAL: a NULL pointer. */
int uc_ddc_carrier_tables(float coarse[2048], float fine[2048]);

/* The outputs of a call: the first absolute output index *p_first = ceil(first / decim) and their number *count (0 where no
 * multiple of decim lies in first .. first + n_samples - 1), as uc_rate_span does for the rate converter.  -EINVAL: a NULL
 * pointer, decim not in 1 .. 64, first + n_samples > 2^64. */
int uc_ddc_outputs(uint64_t first, size_t n_samples, int decim, uint64_t* p_first, size_t* count);

/* The number of outputs of one unit of the kernel's work (a span) at this decimation: where a call's outputs are cut among
 * workgroups (after every uc_ddc_span(decim) outputs, counted from element 0); for tests of the seams.  -EINVAL: decim not in
 * 1 .. 64. */
int uc_ddc_span(int decim);

/* The definition in plain C for one row: n samples of `in` (float or int32 by `dtype`), the first of them with the absolute
 * index `first`, against the carrier (step, phase0) through `taps` (n_taps floats), decimated by decim -> the outputs that
 * uc_ddc_outputs(first, n, decim) names, as I, Q pairs or as I alone by out_format; state[128] is read and brought up to
 * date; needs no GPU.  -EINVAL: a NULL pointer, n == 0, n_taps not in 1 .. 128, decim not in 1 .. 64, an unknown dtype or
 * format, a tap that is not finite, first + n > 2^63; -ENOMEM. */
int uc_ddc_filter_row(const float* taps, int n_taps, int decim, const void* in, int dtype, size_t n, uint64_t first, uint32_t step,
                      uint32_t phase0, float state[128], float* out, int out_format);

/* An object on one device, without tap sets.  -EINVAL: out is NULL; -ENODEV ("no CPU path") when no GPU is visible. */
int uc_ddc_create(int device, uc_ddc** out);
/* Waits for the device, and with it for every call of the object on whatever stream it was given (a call that stages
 * nothing leaves no event to wait for), then frees it.  NULL is allowed. */
void uc_ddc_destroy(uc_ddc* ddc);

/* Uploads n_sets tap sets of n_taps taps each (taps: n_sets x n_taps floats on the host) and the decimation; they replace the
 * object's.  Synchronous: it waits for the device before it writes, so no call in flight reads half a table.  All or
 * nothing: a refused call leaves the object's sets and decimation as they were.  -EINVAL: a NULL pointer, n_sets not in
 * 1 .. 256, n_taps not in 1 .. 128, decim not in 1 .. 64, a tap that is not finite. */
int uc_ddc_set_taps(uc_ddc* ddc, const float* taps, size_t n_sets, int n_taps, int decim);

/* Converts n_samples samples, the first of them with the absolute index `first`, into n_rows output rows.  in_dev (n_in_rows
 * rows, float or int32 by in_dtype), state_dev (n_in_rows x 128 floats, in and out: memory the caller owns) and out_dev
 * (n_rows rows of floats: 2 per output for UC_DDC_OUT_IQ, 1 for UC_DDC_OUT_I) are device memory of the object's device;
 * input row i starts at in_dev + i * in_stride, output row r at out_dev + r * out_stride; strides are in elements (floats),
 * 0 means n_samples and the row's stored floats respectively.  row_map, set_index, step and phase0 are host arrays of
 * n_rows uint32 each, or NULL (row r, set 0, step 0, phase 0); they are read before the call returns.  Asynchronous on
 * hip_stream (a hipStream_t, or NULL): the conversion, and behind it on the same stream the launch that brings the states
 * up to date; the caller's current HIP device is restored.  Any 4-byte alignment and any n_samples: I, Q pairs leave as
 * 8-byte stores where pointer and stride put the rows on 8 bytes, as dwords otherwise.  Every check and allocation comes
 * before the first launch: a refused call (negative errno) has enqueued nothing and leaves the object usable.  -EINVAL: a
 * NULL pointer (ddc, in_dev, state_dev, out_dev); a zero count; n_rows or n_in_rows > 2^32 - 1; no taps uploaded; an unknown
 * dtype or format; in_stride smaller than n_samples, out_stride smaller than the row's stored floats, or either larger than
 * 2^40; first + n_samples > 2^63; a pointer that is not a multiple of 4; in_dev, state_dev or out_dev not device memory of
 * the object's device; row_map[r] >= n_in_rows; n_rows > n_in_rows without a row_map; set_index[r] >= the number of sets;
 * out_dev or state_dev overlapping in_dev or each other.  One thread at a time per object; not capturable into a graph. */
int uc_ddc_run(uc_ddc* ddc, const void* in_dev, int in_dtype, size_t n_in_rows, size_t in_stride, size_t n_rows, size_t n_samples,
               uint64_t first, const uint32_t* row_map, const uint32_t* set_index, const uint32_t* step, const uint32_t* phase0,
               float* state_dev, float* out_dev, int out_format, size_t out_stride, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
