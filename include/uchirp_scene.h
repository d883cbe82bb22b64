/* uchirp_scene.h -- C-ABI of libuchirp_scene.so: the acoustic scene renderer of the chirp modem.
 *
 * uc_link_transmit (uchirp_link.h) gives every microphone one arrival of one transmission.  A scene gives every
 * microphone a list of PATHS: each path is one arrival of one of the scene's transmissions, with its own gain (negative:
 * a phase-inverting reflection), lead time and clock offset.  A direct path and its echoes, several transmitters talking
 * over each other, an array that hears one transmission at different leads: one call renders the sum, plus noise drawn
 * once per microphone, in one pass into the device buffer the receivers of uchirp.h read in place.
 *
 * The library stands alone: it links neither libuchirp_link.so nor libuchirp.so; from uchirp_link.h it takes the types
 * (uc_link_config) and the UC_LINK_DTYPE_* / UC_LINK_MAX_TEXT values only.  There is no CPU path.
 *
 * Definition of sample j (absolute index, j = first_sample + i) of microphone m, whose paths are p_0, p_1, ...
 * (paths[first_path] .. paths[first_path + n_paths - 1], in that order):
 *
 *   y[m][j] = ( x(p_0; j) + x(p_1; j) + ... ) + sigma_m * z(seed, m, j)
 *
 *   x(p; j)  the signal term of uchirp_link.h's definition with amplitude = p.gain, lead_samples = p.lead_samples,
 *            ppm = p.ppm and the text of transmission p.tx: a float, +0.0f where the path is silent
 *   sum      in float, in the order the paths are listed, starting from the first path's value; 0 without paths
 *   z        the noise of uchirp_link.h: Philox4x32-10 keyed by seed, counter = (j / 4 low, j / 4 high, m low, m high),
 *            Box-Muller: the microphone index stands where the link has the stream index; one draw per microphone
 *   output   converted to `dtype` as uc_link_transmit does
 *
 * so a microphone with ONE path is, bit for bit, stream m of uc_link_transmit with the same text, amplitude, lead, ppm,
 * sigma and seed; and a value depends on (seed, m, j, the microphone's paths, their texts) only, never on the launch
 * geometry nor on how a recording is cut into calls (first_sample).  Each path is within 8 float ulp of its own peak
 * |gain| * sqrt 2 of the definition; each addition rounds once.
 *
 * Reach and shift are uchirp_link.h's: the bound holds at every position uc_scene_render accepts (first_sample <= 2^52 =
 * UC_LINK_MAX_FIRST_SAMPLE, n_samples <= 2^40 = UC_LINK_MAX_SAMPLES, any finite lead_samples, |ppm| <= 200; beyond them
 * -EINVAL), because every path's time comes from the integer distance of the sample to the path's own origin
 * (uc_link_frame_origin of uchirp_link.h states the three numbers; this library derives them with the same code).  A scene
 * whose paths all have ppm = 0 is a function of j - lead_samples per path: one integer S added to every lead_samples and
 * to first_sample, where each sum is a double and first_sample + S <= 2^52, changes no bit of the signal terms.
 */
#ifndef UCHIRP_SCENE_H
#define UCHIRP_SCENE_H

#include <stddef.h>
#include <stdint.h>

#include "uchirp_link.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UC_SCENE_ABI_VERSION 1

#define UC_SCENE_MAX_PATHS 16 /* per microphone */

typedef struct uc_scene uc_scene;

/* one arrival of one transmission (24 bytes) */
typedef struct uc_scene_path {
  double lead_samples; /* silence in front of the frame, in samples of fs_out (fractional) */
  float gain;          /* A of this arrival: its peak is |A| * sqrt 2; negative inverts the phase */
  float ppm;           /* clock offset of the receiver against this transmitter, parts per million */
  uint32_t tx;         /* index of the transmission (< n_tx) */
  uint32_t reserved;   /* 0 */
} uc_scene_path;

/* one microphone (16 bytes): paths[first_path .. first_path + n_paths - 1]; ranges of microphones may overlap */
typedef struct uc_scene_mic {
  uint32_t first_path;
  uint32_t n_paths;  /* 0 .. UC_SCENE_MAX_PATHS; 0: noise only */
  float sigma;       /* standard deviation of the added white Gaussian noise (0: none) */
  uint32_t reserved; /* 0 */
} uc_scene_mic;

int uc_scene_abi_version(void);
/* text of the calling thread's last error ("" if none) */
const char* uc_scene_last_error(void);
/* the values of uc_link_default_config */
int uc_scene_default_config(uc_link_config* cfg);
/* -ENODEV ("no CPU path") when no GPU is visible; -EINVAL for a config that is not a frame format */
int uc_scene_create(int device, const uc_link_config* cfg, uc_scene** out);
/* Waits for every call of the object still in flight, on whatever streams they were given (each call is ordered behind the
 * call two before it, so the events of the last two cover all), then frees it.  NULL is allowed. */
void uc_scene_destroy(uc_scene* scene);

/* Renders samples [first_sample, first_sample + n_samples) of every microphone: microphone m to
 * out_dev + m * stride_elems (stride_elems 0: n_samples), elements of `dtype` (UC_LINK_DTYPE_*).
 * text (n_tx x text_stride bytes), text_len (n_tx), paths (n_paths) and mics (n_mics) are HOST arrays: copied into a
 * pinned buffer of the scene before the call returns (the caller may reuse them at once) and from there to the device
 * on hip_stream.  out_dev is device memory of the scene's device.  Asynchronous on hip_stream (a hipStream_t, or NULL).
 * Every argument is checked and every buffer is sized before anything is enqueued: a refused call (negative errno) has
 * enqueued nothing and leaves the scene usable.  -EINVAL: a path's tx >= n_tx; a microphone's first_path + n_paths
 * beyond n_paths of the call, or its n_paths > UC_SCENE_MAX_PATHS; text_len > text_stride; text_stride >
 * UC_LINK_MAX_TEXT; lead_samples, gain, ppm or sigma not finite, sigma < 0; an unknown dtype; a NULL array whose count
 * is not zero; n_mics or n_samples 0; stride_elems < n_samples; out_dev not device memory.
 * One thread at a time per scene; not capturable into a graph.  The scene owns two staging buffers and uses them in
 * turn, so the host runs up to two calls ahead of hip_stream. */
int uc_scene_render(uc_scene* scene, const uint8_t* text, size_t text_stride, const uint32_t* text_len, size_t n_tx,
                    const uc_scene_path* paths, size_t n_paths, const uc_scene_mic* mics, size_t n_mics, void* out_dev, int dtype,
                    double fs_out, uint64_t first_sample, size_t n_samples, size_t stride_elems, uint64_t seed, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
