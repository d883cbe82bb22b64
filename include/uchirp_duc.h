/* uchirp_duc.h -- C-ABI of libuchirp_duc.so: the up-converter of the chirp modem (interpolate, FIR and mix many I/Q rows
 * onto carriers), the counterpart of the down-converter of uchirp_ddc.h.
 *
 * The reference's I/Q modulation (simulation/IQ_modulation.ipynb: carrier_IQ, chirp_x_carrier; simulation/dsp.py;
 * generator/ChirpGeneratorIQmodulation.ipynb) multiplies a base-band pair I, Q by the cosine and the sine of a carrier and
 * adds the products: cos((wc - wb) t) = I cos wc t + Q sin wc t with I + jQ = e^{j wb t}; its generator writes the sum as int16
 * PCM.  uc_duc_run is that stage for many rows at once: n_rows output rows, each the sum of n_chan channels, a channel one
 * base-band input row (I, Q float pairs -- what uc_ddc_run writes as UC_DDC_OUT_IQ -- or I alone) interpolated by 1 .. 64
 * through a polyphase FIR, times the carrier of a 32-bit phase accumulator, as floats or as int16 PCM (what uc_rate_convert
 * reads as UC_RATE_DTYPE_I16).  The history of every input row lives in memory the caller owns, so a stream is converted block
 * by block; with row_map, set_index, step and phase0 one base-band row goes onto k carriers of one loudspeaker in one call.
 * It is the sign that uc_ddc_run undoes: behind its low-pass the down-converter returns (I + jQ) / 2.
 *
 * The library stands alone: it needs no symbol of the other libraries.  There is no CPU path behind uc_duc_run:
 * uc_duc_create fails without a GPU.  uc_duc_filter_row, uc_duc_sum_row, uc_duc_span and uc_duc_carrier_tables are pure host
 * arithmetic and work anywhere.
 *
 * DEFINITION  (uchirp/duc.py holds it in numpy float32: `emulate32`; uc_duc_filter_row and uc_duc_sum_row hold it in plain C)
 *
 * The input sample z[m] = (i, q):
 *   UC_DUC_IN_IQ   interleaved float pairs i, q.
 *   UC_DUC_IN_I    floats i; the Q chain is not computed.
 * A float that is not finite (NaN, +-Inf) reads as +0.  Denormals are kept everywhere: on input, in the products, in the
 * sums and on output.
 *
 * The taps: a set is a prototype of n_taps = K L floats h at the OUTPUT rate, K = 1 .. UC_DUC_MAX_PHASE_TAPS taps per phase,
 * L = 1 .. UC_DUC_MAX_INTERP the interpolation, n_taps <= UC_DUC_MAX_TAPS; one (K, L) per object.  The caller pads a
 * prototype to a multiple of L.  K is part of the definition: a set padded with zero taps gives +0 where the shorter one
 * gives -0.
 *
 * The filter: the output with the absolute index n (uint64) has m = n div L and rho = n mod L.  With ai = +0, for
 * k = 0 .. K - 1:
 *   ai = fmaf(h[rho + k L], i[m - k], ai)
 * and the same chain aq over q, in this order of k.
 *
 * The carrier of a channel is the down-converter's, bit for bit (uchirp_ddc.h), at the OUTPUT index: a 32-bit phase
 * accumulator with step and phase0 (uint32),
 *   phi = (phase0 + step * n) mod 2^32,
 * whatever the cut of the row into calls.  The top 10 bits of phi index the coarse table, 1024 pairs (cc, sc) = (cos, sin)
 * of 2 pi i / 2^10; the next 10 bits index the fine table, 1024 pairs (cf, sf) of 2 pi f / 2^20; the low 12 bits are
 * dropped.  Then, every operation ONE correctly rounded float32 operation and nothing fused,
 *   c = (cc * cf) - (sc * sf)            s = (sc * cf) + (cc * sf)
 * The tables are part of the definition: computed in double and rounded to float; uc_duc_carrier_tables hands them out, and
 * they equal uc_ddc_carrier_tables' to the bit.  With step 0 and phase0 0 the carrier is exactly (1, 0): the call is then a
 * plain interpolating FIR bank.  A negative frequency is the two's-complement step.
 *
 * The mixer, nothing fused: y = (ai * c) + (aq * s) for UC_DUC_IN_IQ, two rounded products and one rounded sum; y = ai * c
 * for UC_DUC_IN_I.
 *
 * Channels: output row r is ((y0 + y1) + y2) + ... over its n_chan channels, 1 .. UC_DUC_MAX_CHAN, in channel order, every
 * sum rounded once.  One channel is y0 itself: no +0 is added, so -0 survives.
 *
 * Output formats: UC_DUC_OUT_F32 stores the float.  UC_DUC_OUT_I16 takes rintf (ties to even) and clamps to -32768 .. 32767;
 * a NaN stores 0.  clip_dev (optional) gains, per output row, the number of that row's outputs in this call whose rounded
 * value lay outside int16 or was NaN (integer atomics: the count does not depend on the order).
 *
 * Positions: a call carries `first`, the absolute index of in[0] at the INPUT rate, shared by all rows, and n_samples inputs;
 * it writes exactly the n_samples L outputs n = first L .. (first + n_samples) L - 1, the first of them at element 0 of the
 * output row.  (first + n_samples) L may not exceed 2^63.
 *
 * The state: per INPUT row the UC_DUC_STATE_SAMPLES = 128 input samples in front of `first`, oldest first, in the input's
 * format (256 floats for UC_DUC_IN_IQ, 128 for UC_DUC_IN_I; what was not finite is stored as +0).  All zeros is a filter at
 * rest.  Channels that share an input row share its state.  A call of fewer than 128 samples shifts the state.
 *
 * An output value depends on its channels' samples, states, taps, steps, phases and position only, never on the grid, the
 * other rows, alignment, or how the row is cut into calls.  So uc_duc_run, uc_duc_filter_row + uc_duc_sum_row and `emulate32`
 * give the same bits.
 *
 * BANKS
 *
 * An object holds up to UC_DUC_MAX_SETS tap sets of one (K, L) (uc_duc_set_taps).  Channel j of output row r is entry
 * r n_chan + j of row_map (NULL: input row r n_chan + j), set_index (NULL: set 0), step (NULL: 0) and phase0 (NULL: 0).  One
 * base-band row on k carriers of one loudspeaker is one call with n_in_rows = 1, n_rows = 1, n_chan = k and row_map all 0.
 *
 * OUT OF SCOPE: taps or channel counts that differ between the rows of a call; DFSDM-word input; non-integer ratios
 * (uc_rate_convert does them); more than 16 channels, 128 taps per phase or 2048 prototype taps; a gain per channel (scale
 * the taps); dither or noise shaping in front of int16; capture into a graph; an overlap-save form for long prototypes: it
 * would change the bits.  The other direction is uchirp_ddc.h.
 */
#ifndef UCHIRP_DUC_H
#define UCHIRP_DUC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UC_DUC_ABI_VERSION 1

#define UC_DUC_IN_IQ 0 /* interleaved float pairs I, Q */
#define UC_DUC_IN_I 1  /* floats: I alone */

#define UC_DUC_OUT_F32 0
#define UC_DUC_OUT_I16 1 /* int16 PCM: rintf, clamped */

#define UC_DUC_MAX_PHASE_TAPS 128 /* K */
#define UC_DUC_MAX_INTERP 64      /* L */
#define UC_DUC_MAX_TAPS 2048      /* K L */
#define UC_DUC_MAX_SETS 256
#define UC_DUC_MAX_CHAN 16
#define UC_DUC_STATE_SAMPLES 128 /* the input samples in front of `first`, oldest first */
#define UC_DUC_TABLE_WORDS 2048  /* 1024 (cos, sin) pairs */

typedef struct uc_duc uc_duc;

int uc_duc_abi_version(void);
/* text of the calling thread's last error ("" if none) */
const char* uc_duc_last_error(void);

/* The carrier's tables: coarse[2 i], coarse[2 i + 1] = cos, sin of 2 pi i / 2^10 and fine[2 f], fine[2 f + 1] = cos, sin of
 * 2 pi f / 2^20, computed in double and rounded to float: the down-converter's.  -EINVAL: a NULL pointer. */
int uc_duc_carrier_tables(float coarse[2048], float fine[2048]);

/* The number of outputs of one unit of the kernel's work (a span) at this interpolation, (2048 div interp) * interp: where
 * a call's outputs are cut among workgroups (after every uc_duc_span(interp) outputs, counted from element 0); for tests
 * of the seams.  -EINVAL: interp not in 1 .. 64. */
int uc_duc_span(int interp);

/* One channel of the definition in plain C: n samples of `in` (I, Q pairs or I alone by in_format), the first of them with
 * the absolute index `first`, through `taps` (k_taps * interp floats), against the carrier (step, phase0) -> the n * interp
 * floats y of the outputs first * interp .. (first + n) * interp - 1 in out_f32; state (256 floats for UC_DUC_IN_IQ, 128 for
 * UC_DUC_IN_I) is read and brought up to date; needs no GPU.  -EINVAL: a NULL pointer, n == 0, k_taps not in 1 .. 128, interp
 * not in 1 .. 64, k_taps * interp > 2048, an unknown format, a tap that is not finite, (first + n) * interp > 2^63; -ENOMEM. */
int uc_duc_filter_row(const float* taps, int k_taps, int interp, const void* in, int in_format, size_t n, uint64_t first, uint32_t step,
                      uint32_t phase0, float* state, float* out_f32);

/* The definition's sum and output stage in plain C: out[i] = ((y[0][i] + y[1][i]) + ...) over n_chan rows of n floats, as
 * floats or as int16 by out_format; *clipped (or NULL) gains the number of int16 outputs whose rounded value lay outside
 * int16 or was NaN.  -EINVAL: a NULL pointer (y, a y[j], out), n == 0, n_chan not in 1 .. 16, an unknown format. */
int uc_duc_sum_row(const float* const* y, int n_chan, size_t n, void* out, int out_format, uint32_t* clipped);

/* An object on one device, without tap sets.  -EINVAL: out is NULL; -ENODEV ("no CPU path") when no GPU is visible. */
int uc_duc_create(int device, uc_duc** out);
/* Waits for the device, and with it for every call of the object on whatever stream it was given (a call that stages
 * nothing leaves no event to wait for), then frees it.  NULL is allowed. */
void uc_duc_destroy(uc_duc* duc);

/* Uploads n_sets prototypes of k_taps * interp taps each (taps: n_sets x k_taps * interp floats on the host); they replace
 * the object's.  Synchronous: it waits for the device before it writes, so no call in flight reads half a table.  All or
 * nothing: a refused call leaves the object's sets, K and L as they were.  -EINVAL: a NULL pointer, n_sets not in 1 .. 256,
 * k_taps not in 1 .. 128, interp not in 1 .. 64, k_taps * interp > 2048, a tap that is not finite. */
int uc_duc_set_taps(uc_duc* duc, const float* taps, size_t n_sets, int k_taps, int interp);

/* Converts n_samples input samples, the first of them with the absolute index `first`, into n_rows output rows of n_samples *
 * interp outputs, each the sum of n_chan channels.  in_dev (n_in_rows rows of floats: 2 per sample for UC_DUC_IN_IQ, 1 for
 * UC_DUC_IN_I), state_dev (n_in_rows x 128 samples of the same format, in and out: memory the caller owns), out_dev (n_rows
 * rows of floats or int16 by out_format) and clip_dev (NULL, or n_rows uint32, in and out; checked but left as it is by a call
 * that writes floats) are device memory of the object's
 * device; input row i starts at in_dev + i * in_stride floats, output row r at out_dev + r * out_stride elements; 0 means the
 * row's own length.  row_map, set_index, step and phase0 are host arrays of n_rows * n_chan uint32 each, or NULL; they are
 * read before the call returns.  Asynchronous on hip_stream (a hipStream_t, or NULL): the conversion, and behind it on the
 * same stream the launch that brings the states up to date; the caller's current HIP device is restored.  Any 4-byte
 * alignment of the floats, any 2-byte alignment of int16 and any stride: I, Q pairs are read by 8-byte loads where pointer
 * and stride put the rows on 8 bytes; int16 leave as 8-byte stores of four and 4-byte stores of two where they lie so, as
 * single values otherwise.  Every check and allocation comes before the first launch: a refused call (negative errno) has
 * enqueued nothing and leaves the object usable.  -EINVAL: a NULL pointer (duc, in_dev, state_dev, out_dev); a zero count;
 * n_rows or n_in_rows > 2^32 - 1; n_chan not in 1 .. 16; no taps uploaded; an unknown format; in_stride smaller than the
 * row's floats, out_stride smaller than n_samples * interp, or either larger than 2^40; (first + n_samples) * interp > 2^63;
 * in_dev, state_dev or clip_dev not a multiple of 4, out_dev not a multiple of 4 (floats) or 2 (int16); in_dev, state_dev,
 * out_dev or clip_dev not device memory of the object's device; row_map[i] >= n_in_rows; n_rows * n_chan > n_in_rows without
 * a row_map; set_index[i] >= the number of sets; out_dev, state_dev or clip_dev overlapping in_dev or each other.  One thread
 * at a time per object; not capturable into a graph. */
int uc_duc_run(uc_duc* duc, const void* in_dev, int in_format, size_t n_in_rows, size_t in_stride, size_t n_rows, int n_chan,
               size_t n_samples, uint64_t first, const uint32_t* row_map, const uint32_t* set_index, const uint32_t* step,
               const uint32_t* phase0, float* state_dev, void* out_dev, int out_format, size_t out_stride, uint32_t* clip_dev,
               void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
