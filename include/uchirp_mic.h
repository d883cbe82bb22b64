/* uchirp_mic.h -- C-ABI of libuchirp_mic.so: the MEMS-microphone model of the chirp modem (sample rows at 78 125 Hz to the
 * microphones' 1-bit PDM streams at 2.5 MHz).
 *
 * The chain this project serves starts at the microphones' PDM bits: the receivers take UC_DTYPE_PDM, uc_dfsdm_sinc5_streams
 * decimates thousands of microphones.  uc_mic_modulate is the stage in front of them: n_rows rows of samples in, the same
 * rows as packed PDM words out, one word per sample, through a second-order delta-sigma modulator in integer arithmetic, in
 * device memory that uc_receive_streams[_next] (UC_DTYPE_PDM) and uc_dfsdm_sinc5_streams read in place.
 *
 * The library stands alone: it needs no symbol of the other ten libraries.  There is no CPU path behind uc_mic_modulate:
 * uc_mic_create fails without a GPU.  uc_mic_quantise and uc_mic_modulate_row are pure host arithmetic and work anywhere.
 *
 * DEFINITION  (uchirp/mic.py holds it in numpy integers: `model`)
 *
 * All state and arithmetic is int32 in two's complement with wrap-around, so the definition is total: every input and every
 * state has one output.  Y = 2^25.  A row carries a state of 4 int32 words {prev, s1, s2, 0}: the previous quantised sample
 * and the two integrators.  All zeros is a microphone that starts.  The fourth word is reserved: it is not read, and 0 is
 * written.
 *
 * Quantise sample j of the row to q, |q| <= 2^23 - 1:
 *   UC_MIC_DTYPE_F32   v = x * scale, one float multiply; `scale` is a finite positive float of the object.  Scale 1 takes
 *                      floats in units of the 24-bit LSB (what uc_link_transmit means by its I32 output), scale 8388607
 *                      takes floats in [-1, 1].  q = rintf(v), to nearest even, clamped to +-(2^23 - 1).  NaN reads as 0.
 *   UC_MIC_DTYPE_I32   (DFSDM words) q = word >> 8 (arithmetic shift), clamped to +-(2^23 - 1).  `scale` is not applied.
 *
 * Interpolate and modulate, for b = 0 .. 31; the interpolation is causal and linear, from the previous sample to this one:
 *   d = q - prev
 *   u = 2 prev + ((d (b + 1)) >> 4)      arithmetic shift; u = 2 q at b = 31; |u| <= Y / 2: half scale
 *   y = (s2 >= 0) ? +Y : -Y
 *   s1 += u - y;   s2 += s1 - y
 *   bit b of the output word = (y > 0)   bit t of the stream is bit (t & 31) of word t >> 5: uc_dfsdm_sinc5's packing
 * After bit 31, prev = q.
 *
 * One output word per input sample.  A word depends on its row's samples and the row's state only, never on the grid, the
 * other rows, or how the row is cut into calls.
 *
 * What follows from it:
 *   - The loop's signal transfer is one bit of delay exactly: s2 after bit t is the double sum of u - y up to t plus the
 *     single sum, so the bits are u delayed by one bit plus the quantisation error differenced twice.
 *   - Behind uc_dfsdm_sinc5_streams the words are 1/2 * sinc^2(f / 78 125) * (the sinc^5's own response) of the input,
 *     about 2.45 samples late: sample j is reached at bit 32 j + 31, one bit for the loop, and the sinc^5's centre lies
 *     77.5 bits before the end of its last word.  (The factor 1/2 is the half scale of u: a full-scale input modulates
 *     half of the bit density's range, where a second-order loop is stable.)
 *   - Silence gives the words 0x99999999, and the sinc^5 of that is 0 exactly.
 *   - With |q| <= 2^23 - 1 and a state reached from zeros the integrators stay within a few Y (measured on full-scale
 *     chirps, tones, noise, DC and alternating inputs: |s1| <= 2.25 Y, |s2| <= 4.25 Y); int32 holds 64 Y.
 *
 * OUT OF SCOPE: microphone noise, DC offset and the acoustic overload point of a real part; other oversampling ratios than
 * 32 (uc_dfsdm_run reads other ratios); higher-order loops; PDM bit orders other than uc_dfsdm_sinc5's; capture into a graph.
 */
#ifndef UCHIRP_MIC_H
#define UCHIRP_MIC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UC_MIC_ABI_VERSION 1

#define UC_MIC_DTYPE_I32 0 /* DFSDM words: the 24-bit value in bits 31:8 */
#define UC_MIC_DTYPE_F32 1

#define UC_MIC_Q_MAX 8388607   /* 2^23 - 1 */
#define UC_MIC_Y 33554432      /* 2^25 */
#define UC_MIC_OSR 32          /* bits per sample: one output word */
#define UC_MIC_SILENCE 0x99999999u /* every word of a row of zeros from the zero state */

typedef struct uc_mic uc_mic;

int uc_mic_abi_version(void);
/* text of the calling thread's last error ("" if none) */
const char* uc_mic_last_error(void);

/* The quantiser of the definition for n samples (in: float or int32 by `dtype`); needs no GPU.  `scale` is read for
 * UC_MIC_DTYPE_F32 only.  -EINVAL: a NULL pointer, n == 0, an unknown dtype, a scale that is not finite and positive
 * (UC_MIC_DTYPE_F32). */
int uc_mic_quantise(const void* in, int dtype, float scale, size_t n, int32_t* q_out);

/* The definition in plain C for one row: n quantised samples -> n words; state[4] is read and brought up to date; needs no
 * GPU.  q may hold any int32 (the arithmetic wraps).  -EINVAL: a NULL pointer, n == 0. */
int uc_mic_modulate_row(const int32_t* q, size_t n, int32_t state[4], uint32_t* words_out);

/* An object on one device.  -EINVAL: a scale that is not finite and positive, out is NULL; -ENODEV ("no CPU path") when no
 * GPU is visible. */
int uc_mic_create(int device, float scale, uc_mic** out);
/* Frees the object at once: it owns no device memory, so no call in flight reads anything of it.  NULL is allowed. */
void uc_mic_destroy(uc_mic* mic);

/* Modulates n_samples samples of n_rows rows.  in_dev (float or int32 by in_dtype), state_dev (n_rows x 4 int32, in and out:
 * memory the caller owns, as the `history` of uc_dfsdm_sinc5_streams) and out_dev are device memory of the object's device;
 * row r starts at in_dev + r * in_stride and out_dev + r * out_stride; strides are in elements, 0 means n_samples.
 * Asynchronous on hip_stream (a hipStream_t, or NULL); the caller's current HIP device is restored.  The call reads no host
 * array: all it needs travels as kernel arguments, so nothing is staged and calls in a row do not wait for each other on the
 * host.  Any 4-byte alignment and any n_samples: 16-byte accesses where pointer and stride allow them, dword accesses
 * otherwise.  Every argument is checked before anything is enqueued: a refused call (negative errno) has enqueued nothing
 * and leaves the object usable.  -EINVAL: a NULL pointer; a zero count; n_rows > 2^32 - 1; an unknown dtype; a stride
 * smaller than n_samples or larger than 2^40; a pointer that is not a multiple of 4; in_dev, state_dev or out_dev not device
 * memory of the object's device; out_dev or state_dev overlapping in_dev or each other.  One thread at a time per object;
 * not capturable into a graph. */
int uc_mic_modulate(uc_mic* mic, const void* in_dev, int in_dtype, size_t n_rows, size_t n_samples, size_t in_stride,
                    int32_t* state_dev, uint32_t* out_dev, size_t out_stride, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
