/* uchirp_dfsdm.h -- C-ABI of libuchirp_dfsdm.so: the DFSDM filter in every configuration of the peripheral (rows of packed
 * 1-bit PDM words to rows of 24-bit filter words: FastSinc or Sinc1..5, any ratio, integrator, right shift and offset).
 *
 * The chain this project serves starts at the microphones' PDM bits.  uc_dfsdm_sinc5 / uc_dfsdm_sinc5_streams of libuchirp.so
 * are the peripheral in ONE configuration -- SINC5, oversampling 32, integrator 1, right shift 2: receiver/Src/dfsdm.c --
 * and stay the fast path for it.  Six of the reference's nine firmware projects that set the peripheral up run SINC3, and
 * three different clock dividers occur; a 64x microphone or an integrator used to reach audio rates is another setting again.  uc_dfsdm_run is the peripheral with
 * its registers open: n_rows rows of PDM words in, the rows' filter words out, in device memory, the filter's state carried
 * between calls in memory the caller owns.
 *
 * The library stands alone: it needs no symbol of the other libraries.  There is no CPU path behind uc_dfsdm_run:
 * uc_dfsdm_create fails without a GPU.  uc_dfsdm_check, uc_dfsdm_gain, uc_dfsdm_plan and uc_dfsdm_filter_row are pure host
 * arithmetic and work anywhere.  The input is bits: there are no non-finite samples here.
 *
 * DEFINITION  (uchirp/dfsdm.py holds it in numpy: `model`)
 *
 * A configuration is {order, ratio R, integrator I, shift, offset}: order 0 is FastSinc, 1 .. 5 are Sinc1 .. Sinc5; R is
 * 1 .. 1024, I is 1 .. 256, shift is 0 .. 31, offset is -2^23 .. 2^23 - 1 (stm32l4xx_hal_dfsdm.h:460-465, 796-797, 847-848).
 * Let N = order, N = 2 for FastSinc.  The full-scale gain is G = R^N I, for FastSinc 2 R^2 I.  A configuration is accepted
 * only if G <= 2^31 - 1, the peripheral's own 32-bit limit (the data sheet's Sinc5 <= 73, Sinc4 <= 215 at I = 1); everything
 * else is -EINVAL.
 *
 * All state and arithmetic is int32 in two's complement with wrap-around, so the definition is total: every input and every
 * state has one output.  A row carries a state of 16 int32 words: integ[5] (words 0 .. 4), comb[5] (5 .. 9), fast[2]
 * (10, 11), acc (12) and three reserved words (13 .. 15: not read, 0 is written).  Stages that the order does not run, and
 * fast[] outside FastSinc, are neither read nor written.  All zeros is the peripheral just enabled.
 *
 * Bit t of a row is bit (t & 31) of word t >> 5 (uc_dfsdm_sinc5's packing); a 1 is s = +1, a 0 is s = -1.
 *   1. per bit:  integ[0] += s; then integ[k] += integ[k - 1] for k = 1 .. N - 1, each on the stage before it as already
 *      brought up to date.
 *   2. at every R-th bit of the row, counted from its zero state:  v = integ[N - 1]; for k = 0 .. N - 1: d = v - comb[k],
 *      comb[k] = v, v = d.  FastSinc then forms w = v + fast[1], fast[1] = fast[0], fast[0] = v, v = w (the factor
 *      1 + z^(-2R)).  Then acc += v.
 *   3. at every I-th such value:  y = acc (signed), acc = 0; the output word is
 *      clip((y >> shift) - offset, -2^23, 2^23 - 1) * 256: the 24-bit result in bits 31:8, what every library here reads
 *      as I32.  The shift is arithmetic.
 *
 * A call consumes whole words.  Where a row stands between the R and I boundaries is NOT state: the caller passes
 * words_before, the words the row has consumed since its zero state, one value for all rows of a call.  A call of n_words
 * gives   n_out = floor(32 (words_before + n_words) / (R I)) - floor(32 words_before / (R I))   words per row.
 *
 * What follows from it:
 *   - From the zero state the outputs are the FIR of the bits with a zero past: taps = the N-fold convolution of R ones
 *     (for FastSinc: of two such boxcars and {1, 0 .. 0, 1} of length 2 R + 1), summed over I values, taken at every
 *     R I-th bit.  G <= 2^31 - 1 is what keeps that sum inside int32; the wrap-around in between cancels.
 *   - With {5, 32, 1, 2, 0} the outputs 4, 5, ... are uc_dfsdm_sinc5 of the same words exactly.
 *   - The words 0x99999999 of a silent uc_mic_modulate give 0 exactly once the filter is full, where R is a multiple of 4.
 *   - Behind uc_mic_modulate and through SINC3 / 32 the words are 1/2 sinc^2(f / 78 125) times the sinc^3's own response of
 *     the microphone's input (DESIGN.md has the measured deviation).
 *
 * PARALLELISM is over rows only: a row is a recurrence and runs on ONE lane of the GPU, so one long recording uses one lane
 * while 65 536 rows fill the chip.  Cutting a row in time (by FIR warm-up segments) is out of scope.
 *
 * OUT OF SCOPE: the peripheral's parallel-data input, watchdog, extremes detector and injected conversions; bit orders other
 * than uc_dfsdm_sinc5's; cutting one row across lanes; capture into a graph.
 */
#ifndef UCHIRP_DFSDM_H
#define UCHIRP_DFSDM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UC_DFSDM_ABI_VERSION 1

#define UC_DFSDM_ORDER_FASTSINC 0 /* orders 1 .. 5 are Sinc1 .. Sinc5 */
#define UC_DFSDM_ORDER_MAX 5
#define UC_DFSDM_RATIO_MAX 1024
#define UC_DFSDM_INTEGRATOR_MAX 256
#define UC_DFSDM_SHIFT_MAX 31
#define UC_DFSDM_OFFSET_MIN (-8388608) /* -2^23 */
#define UC_DFSDM_OFFSET_MAX 8388607    /* 2^23 - 1 */
#define UC_DFSDM_GAIN_MAX 2147483647   /* 2^31 - 1 */
#define UC_DFSDM_STATE_WORDS 16

typedef struct uc_dfsdm_config {
  int32_t order;       /* 0: FastSinc; 1 .. 5: Sinc1 .. Sinc5 */
  uint32_t ratio;      /* R: 1 .. 1024 */
  uint32_t integrator; /* I: 1 .. 256 */
  int32_t shift;       /* 0 .. 31 */
  int32_t offset;      /* -2^23 .. 2^23 - 1 */
} uc_dfsdm_config;

typedef struct uc_dfsdm uc_dfsdm;

int uc_dfsdm_abi_version(void);
/* text of the calling thread's last error ("" if none) */
const char* uc_dfsdm_last_error(void);

/* 0 if the configuration is one of the definition's, else -EINVAL with the reason in uc_dfsdm_last_error: cfg is NULL, a
 * field outside its range, G > 2^31 - 1.  Needs no GPU. */
int uc_dfsdm_check(const uc_dfsdm_config* cfg);
/* G of the definition as it stands (no check of the limit); 0 if cfg is NULL or order, ratio or integrator is outside its
 * range.  Needs no GPU. */
uint64_t uc_dfsdm_gain(const uc_dfsdm_config* cfg);
/* n_out of the definition for a call of n_words behind words_before.  -EINVAL: what uc_dfsdm_check refuses, n_out is NULL,
 * words_before + n_words > 2^58.  n_words may be 0.  Needs no GPU. */
int uc_dfsdm_plan(const uc_dfsdm_config* cfg, uint64_t words_before, uint64_t n_words, uint64_t* n_out);
/* The definition in plain C for one row: n_words words -> *n_out words in out; state[16] is read and brought up to date;
 * needs no GPU.  -EINVAL: what uc_dfsdm_plan refuses, a NULL pointer (out may be NULL where the plan gives 0 outputs),
 * n_words == 0, out_cap smaller than the plan's count (nothing is written then, the state is as it was). */
int uc_dfsdm_filter_row(const uc_dfsdm_config* cfg, const uint32_t* words, size_t n_words, uint64_t words_before, int32_t state[16],
                        int32_t* out, size_t out_cap, size_t* n_out);

/* An object on one device, for one configuration.  -EINVAL: what uc_dfsdm_check refuses, out is NULL; -ENODEV ("no CPU
 * path") when no GPU is visible.  Where R is a multiple of 32 the object owns the word path's tables in device memory. */
int uc_dfsdm_create(int device, const uc_dfsdm_config* cfg, uc_dfsdm** out);
/* Waits until the device is idle (no call stages anything, so a pending call leaves no event to wait for, and it may read
 * the object's tables), then frees the object.  NULL is allowed. */
void uc_dfsdm_destroy(uc_dfsdm* obj);

/* Filters n_words words of n_rows rows.  pdm_dev, state_dev (n_rows x 16 int32, in and out: memory the caller owns) and
 * out_dev are device memory of the object's device; row r starts at pdm_dev + r * in_stride and out_dev + r * out_stride;
 * strides are in words, 0 means dense (n_words, and n_out of uc_dfsdm_plan).  A row of out_dev receives n_out words; what
 * lies behind them is not touched.  A call that gives no output (n_out == 0) is a valid call: it brings the states up to
 * date.  Asynchronous on hip_stream (a hipStream_t, or NULL); the caller's current HIP device is restored.  The call reads
 * no host array: all it needs travels as kernel arguments, so nothing is staged and calls in a row do not wait for each
 * other on the host.  Any 4-byte alignment and any n_words: tiles of 16 words through 16-byte accesses where pointer and
 * stride put every row on 16 bytes, dword accesses otherwise; the words are the same.  Every argument is checked before
 * anything is enqueued: a refused call (negative errno) has enqueued nothing and leaves the object usable.  -EINVAL: a NULL
 * pointer; a zero count; n_rows > 2^32 - 1; words_before + n_words > 2^58; in_stride smaller than n_words, out_stride
 * smaller than n_out, either larger than 2^40; a pointer that is not a multiple of 4; pdm_dev, state_dev or out_dev not
 * device memory of the object's device; out_dev or state_dev overlapping pdm_dev or each other.  One thread at a time per
 * object; not capturable into a graph. */
int uc_dfsdm_run(uc_dfsdm* obj, const uint32_t* pdm_dev, size_t n_rows, size_t n_words, size_t in_stride, uint64_t words_before,
                 int32_t* state_dev, int32_t* out_dev, size_t out_stride, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
