/* uchirp_link.h -- C-ABI of libuchirp_link.so: the link simulator of the chirp modem.
 *
 * One call renders, on the GPU and in one pass, what n_streams microphones receive from n_streams independent
 * transmissions: each stream its own text, amplitude, lead time, clock offset and noise level, written straight into a
 * device buffer that uc_receive_streams / uc_receive_streams_next / uc_process_batch (uchirp.h) read in place.
 *
 * The library stands alone: it does not link libuchirp.so and shares no type with uchirp.h.  There is no CPU path.
 *
 * Definition of sample j (absolute index, j = first_sample + i) of stream s:
 *
 *   signal   tt  = j / fs_out * (1 + ppm * 1e-6) - lead_samples / fs_out          (seconds since the frame began)
 *            idx = floor((tt + 1e-10) / sym_dur),  sym_dur = n_sym / fs_tx,  n_sym = (int)(t_symbol * fs_tx)
 *            tau = max(tt - idx * sym_dur, 0),     t = tau * fs_tx * t_symbol / (n_sym - 1)
 *            symbol idx of the frame: G, n_preamble x H, L, the text's bits MSB first, n_guard x G   (G = silence)
 *            H: f = f0 + k t / 2,  L: f = f1 - k t / 2,  k = (f1 - f0) / t_symbol
 *            x = amplitude * (cos(a) + sin(a)),  a = 2 pi f t - pi / 2;   0 in G and outside the frame
 *   noise    Philox4x32-10, key = seed, counter = (j / 4 low, j / 4 high, s low, s high); word w of the counter belongs
 *            to sample 4 (j / 4) + w;  u = ((word >> 8) + 0.5) * 2^-24;
 *            z0, z1 = sqrt(-2 ln u0) * (cos, sin)(2 pi u1);  z2, z3 the same from u2, u3
 *   output   x + sigma * z, converted to `dtype`
 *
 * so a buffer does not depend on the launch geometry nor on how a recording is cut into calls (first_sample).
 * The device evaluates the phase in turns in double precision, reduces it and takes ONE float sine per sample
 * (cos a + sin a = sqrt 2 sin(a + pi / 4)): within 8 ulp of float at the peak amplitude * sqrt 2 of the definition above.
 *
 * Reach.  The definition is meant in exact arithmetic on the arguments' binary values (1e-6 is the number 10^-6), and the
 * bound holds at every position the calls accept: first_sample <= 2^52 (UC_LINK_MAX_FIRST_SAMPLE), n_samples <= 2^40
 * (UC_LINK_MAX_SAMPLES), any finite lead_samples, |ppm| <= 200; a call beyond them is refused with -EINVAL.  tt is not
 * computed as the difference of two times of the size of j / fs_out, whose error would grow with j (about 10 ulp at
 * j = 2^33, 30 hours at 78 125 Hz), but from an integer distance (uc_link_frame_origin):
 *
 *            origin = the integer nearest to lead_samples / (1 + ppm * 1e-6)      (where the frame begins)
 *            t0     = (origin * (1 + ppm * 1e-6) - lead_samples) / fs_out          (under one sample; summed exactly)
 *            tt     = (j - origin) * ((1 + ppm * 1e-6) / fs_out) + t0
 *
 * Shift.  With ppm = 0 the signal is a function of j - lead_samples alone: adding one integer S to lead_samples and to
 * first_sample, where lead_samples + S is a double and first_sample + S <= 2^52, changes no bit of the signal.  (The noise
 * belongs to the absolute sample index and moves with it.)
 */
#ifndef UCHIRP_LINK_H
#define UCHIRP_LINK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UC_LINK_ABI_VERSION 2 /* 2: uc_link_frame_origin; the reach and the shift property are part of the contract */

/* output formats.  I32 and F32 carry the values of UC_DTYPE_I32 / UC_DTYPE_F32 of uchirp.h. */
#define UC_LINK_DTYPE_I32 0 /* DFSDM words: round-to-nearest-even(x) * 256, the 24-bit sample in bits 31:8 (saturating) */
#define UC_LINK_DTYPE_F32 1 /* float, as is */
#define UC_LINK_DTYPE_I16 3 /* int16, truncated toward zero (what a WAV writer's cast does), saturating */

#define UC_LINK_MAX_TEXT 4096 /* largest text_stride */

#define UC_LINK_MAX_FIRST_SAMPLE (1ull << 52) /* largest first_sample */
#define UC_LINK_MAX_SAMPLES (1ull << 40)      /* largest n_samples */

typedef struct uc_link uc_link;

typedef struct uc_link_config {
  double fs_tx;        /* the transmitter's sample rate: 44100 */
  double t_symbol;     /* nominal symbol time: 0.0262 s -> n_sym = (int)(t_symbol * fs_tx) = 1155 samples at fs_tx */
  double f0, f1;       /* chirp band: 16000 .. 19000 Hz */
  uint32_t n_preamble; /* H symbols in front of the delimiter: 7 */
  uint32_t n_guard;    /* G symbols behind the data: 12 */
} uc_link_config;

typedef struct uc_link_stream {
  double lead_samples; /* silence in front of the frame, in samples of fs_out (fractional) */
  float amplitude;     /* A: the symbol's peak is A * sqrt 2 */
  float sigma;         /* standard deviation of the added white Gaussian noise (0: none) */
  float ppm;           /* clock offset of the receiver against the transmitter, parts per million */
  uint32_t text_len;   /* bytes of this stream's text (<= text_stride) */
} uc_link_stream;

/* what the host derives from one stream's lead_samples, ppm and fs_out (24 bytes) */
typedef struct uc_link_origin {
  int64_t origin; /* the integer nearest to lead_samples / (1 + ppm * 1e-6), ties to even; held to +-2^53 */
  double t0;      /* (origin * (1 + ppm * 1e-6) - lead_samples) / fs_out: seconds since the frame began at sample origin */
  double rate;    /* (1 / fs_out) * (1 + ppm * 1e-6) in double: seconds of transmitter time per output sample */
} uc_link_origin;

int uc_link_abi_version(void);
/* text of the calling thread's last error ("" if none) */
const char* uc_link_last_error(void);
/* the format of the reference transmission: 44100 Hz, 0.0262 s, 16000 .. 19000 Hz, 7 preamble symbols, 12 guard symbols */
int uc_link_default_config(uc_link_config* cfg);
/* The three numbers the kernels take a stream's time from (see "Reach"); pure host arithmetic, needs no GPU.  t0 is within
 * 2 ulp of its rational value for |ppm| <= 200 and |lead_samples| <= 2^53.  -EINVAL: out is NULL; lead_samples or ppm not
 * finite; fs_out not positive and finite. */
int uc_link_frame_origin(double lead_samples, float ppm, double fs_out, uc_link_origin* out);
/* -ENODEV ("no CPU path") when no GPU is visible; -EINVAL for a config that is not a frame format */
int uc_link_create(int device, const uc_link_config* cfg, uc_link** out);
/* Waits for every call of the object still in flight, on whatever streams they were given (each call is ordered behind the
 * call two before it, so the events of the last two cover all), then frees it.  NULL is allowed. */
void uc_link_destroy(uc_link* link);

/* Renders samples [first_sample, first_sample + n_samples) of every stream: stream s to out_dev + s * stride_elems
 * (stride_elems 0: n_samples), elements of `dtype`.
 * text (n_streams x text_stride bytes) and params (n_streams) are HOST arrays: copied into a pinned buffer of the link
 * before the call returns (the caller may reuse them at once) and from there to the device on hip_stream.
 * out_dev is device memory of the link's device.  Asynchronous on hip_stream (a hipStream_t, or NULL).
 * Every argument is checked and every buffer is sized before anything is enqueued: a refused call (negative errno)
 * has enqueued nothing and leaves the link usable.  One thread at a time per link; not capturable into a graph.
 * The link owns two staging buffers and uses them in turn, so the host runs up to two calls ahead of hip_stream: a
 * call blocks the host only while the copy of the call two before it has not yet run (and, once, when a larger call
 * makes a staging buffer grow). */
int uc_link_transmit(uc_link* link, const uint8_t* text, size_t text_stride, const uc_link_stream* params, size_t n_streams,
                     void* out_dev, int dtype, double fs_out, uint64_t first_sample, size_t n_samples, size_t stride_elems,
                     uint64_t seed, void* hip_stream);

/* The raw generator: the 4 words of the counters first_counter .. first_counter + n_counters - 1 of `stream` under
 * `seed`, to out_dev (device memory, 4 * n_counters words).  Asynchronous on hip_stream. */
int uc_link_noise_words(uc_link* link, uint64_t seed, uint64_t stream, uint64_t first_counter, size_t n_counters,
                        uint32_t* out_dev, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
