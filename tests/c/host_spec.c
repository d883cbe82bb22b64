/* host_spec.c -- a plain C99 host of the spectrum analyser (include/uchirp_spec.h, libuchirp_spec.so): counts the frames of
 * a 2 s recording at the receivers' 78 125 Hz (no GPU), then sends three blocks of a 17 kHz tone through uc_spec_run on the
 * GPU as the firmware's fft() would look at them -- Hann window, magnitude / sqrt(N), AC coupling below 1 kHz, 10 log10 --
 * and prints the peak record of each frame: bin 446, the bin next to 17 000 Hz.  Device memory comes from libuchirp.so's
 * helpers for hosts without the HIP headers.
 * Without a GPU uc_spec_create reports the missing device and the program says so (exit code 0). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uchirp.h"
#include "uchirp_spec.h"

#define FS 78125.0
#define TONE 17000.0
#define FRAMES 3
#define N_IN (FRAMES * UC_SPEC_POINTS)

int main(void) {
  static float x[N_IN];
  static float level[FRAMES * UC_SPEC_BINS];
  uc_spec_peak peaks[FRAMES];
  uc_spec_params p;
  uc_spec_info info;
  uc_spec* an = NULL;
  void *in = NULL, *out = NULL, *pk = NULL;
  const double pi = 3.14159265358979323846;
  int rc, i, f, at_446 = 0;

  printf("uc_spec_abi_version %d (header %d)\n", uc_spec_abi_version(), UC_SPEC_ABI_VERSION);
  printf("2 s at 78125 Hz: %lld frames at hop 2048, %lld at hop 512, %lld centred\n", (long long)uc_spec_frames(156250, 0, 2048, 2048),
         (long long)uc_spec_frames(156250, 0, 2048, 512), (long long)uc_spec_frames(156250, -1024, 2048, 512));
  memset(&p, 0, sizeof(p));
  p.frame_len = UC_SPEC_POINTS;
  p.hop = 0;
  p.n_bins = UC_SPEC_BINS;
  p.ac_bins = 27; /* the bins below 1 kHz at 78 125 Hz */
  p.kind = UC_SPEC_DB;
  p.scale = (float)(1.0 / sqrt((double)UC_SPEC_POINTS));
  p.floor = 1e-6f;
  p.db_mul = 10.0f; /* main.c:135 */
  if (uc_spec_plan(&p, 1, N_IN, 0, &info) == 0) {
    printf("hop 0 was not refused\n");
    return 1;
  }
  printf("hop 0 refused: %s\n", uc_spec_last_error());
  p.hop = UC_SPEC_POINTS;
  if (uc_spec_plan(&p, 1, N_IN, 0, &info) || info.n_frames != FRAMES || info.out_elems != FRAMES * UC_SPEC_BINS) {
    printf("uc_spec_plan: %s\n", uc_spec_last_error());
    return 1;
  }
  rc = uc_spec_create(0, &an);
  if (rc) {
    printf("uc_spec_create: %d (%s)\n", rc, uc_spec_last_error());
    return 0;
  }
  for (i = 0; i < N_IN; i++) x[i] = (float)(1000.0 * sin(2.0 * pi * TONE * (double)i / FS));
  if (uc_device_malloc(0, sizeof(x), &in) || uc_device_malloc(0, sizeof(level), &out) || uc_device_malloc(0, sizeof(peaks), &pk) ||
      uc_device_copy(in, x, sizeof(x))) {
    printf("allocation failed: %s\n", uc_last_error());
    return 1;
  }
  rc = uc_spec_run(an, in, UC_SPEC_DTYPE_F32, 1, N_IN, 0, &p, (float*)out, 0, (uc_spec_peak*)pk, NULL);
  if (rc) {
    printf("uc_spec_run: %d (%s)\n", rc, uc_spec_last_error());
    return 1;
  }
  if (uc_device_copy(level, out, sizeof(level)) || uc_device_copy(peaks, pk, sizeof(peaks))) { /* joins the launch */
    printf("uc_device_copy: %s\n", uc_last_error());
    return 1;
  }
  for (f = 0; f < FRAMES; f++) {
    printf("frame %d: %.2f dB at bin %u; bin 0 under the AC coupling %.2f dB\n", f, (double)peaks[f].value, (unsigned)peaks[f].bin,
           (double)level[f * UC_SPEC_BINS]);
    at_446 += peaks[f].bin == 446 && peaks[f].value == level[f * UC_SPEC_BINS + 446] && level[f * UC_SPEC_BINS] == 0.0f;
  }
  printf("tone at %.0f Hz of %.0f Hz: peak at bin 446 (%.1f Hz) in %d of %d frames\n", TONE, FS, 446.0 * FS / UC_SPEC_POINTS, at_446, FRAMES);
  uc_device_free(0, pk);
  uc_device_free(0, out);
  uc_device_free(0, in);
  uc_spec_destroy(an);
  return at_446 == FRAMES ? 0 : 1;
}
