/* host_array.c -- a plain C99 host of the array combiner (include/uchirp_array.h, libuchirp_array.so): renders
 * "Hello World!" for an array of 8 microphones, each at its own fractional lead and with its own noise
 * (libuchirp_scene.so), steers one delay-and-sum beam at the transmitter, and prints what uc_receive_streams
 * (libuchirp.so, the complex-reference receiver) decodes from the beam.  Device memory comes from libuchirp.so's helpers
 * for hosts without the HIP headers.
 * Without a GPU uc_array_create reports the missing device and the program says so (exit code 0). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uchirp.h"
#include "uchirp_array.h"
#include "uchirp_scene.h"

#define MICS 8
#define BLOCK 2048
#define LEAD 30 /* blocks of noise in front: the receiver's mag_mean needs 24 of them */
#define BLOCKS 160

int main(void) {
  const char* msg = "Hello World!";
  const uint32_t len = (uint32_t)strlen(msg);
  const size_t n_samples = (size_t)BLOCKS * BLOCK;
  static const double offset[MICS] = {0.0, 3.25, 7.5, 12.125, 18.75, 22.0, 31.375, 39.5}; /* samples */
  uc_link_config fmt;
  uc_scene_path paths[MICS];
  uc_scene_mic mics[MICS];
  uc_array_tap taps[MICS];
  uc_array_beam beam;
  uc_scene* scene = NULL;
  uc_array* array = NULL;
  uc_config cfg;
  uc_ctx* uc = NULL;
  void *dev = NULL, *out = NULL;
  char text[64];
  uint32_t n_text;
  float probe;
  float coef[UC_ARRAY_COEFS];
  int64_t shift;
  char* nl;
  int rc, m;

  printf("uc_array_abi_version %d (header %d)\n", uc_array_abi_version(), UC_ARRAY_ABI_VERSION);
  if (uc_array_tap_coefficients(2.5, 1.0f, &shift, coef)) {
    printf("uc_array_tap_coefficients: %s\n", uc_array_last_error());
    return 1;
  }
  printf("delay 2.5: shift %d, c[7] = c[8] = %.6f\n", (int)shift, (double)coef[7]);
  rc = uc_array_create(0, &array);
  if (rc) {
    printf("uc_array_create: %d (%s)\n", rc, uc_array_last_error());
    return 0;
  }
  uc_scene_default_config(&fmt);
  rc = uc_scene_create(0, &fmt, &scene);
  if (rc) {
    printf("uc_scene_create: %d (%s)\n", rc, uc_scene_last_error());
    return 1;
  }
  if (uc_default_config(UC_SYNC_CPLX, &cfg) != 0 || uc_create(&cfg, &uc) != 0) {
    printf("uc_create: %s\n", uc_last_error());
    return 1;
  }
  if (uc_device_malloc(0, MICS * n_samples * sizeof(float), &dev) || uc_device_malloc(0, n_samples * sizeof(float), &out)) {
    printf("allocation failed: %s\n", uc_last_error());
    return 1;
  }
  for (m = 0; m < MICS; m++) {
    paths[m].lead_samples = (double)LEAD * BLOCK + 100.25 + offset[m];
    paths[m].gain = 2000.0f;
    paths[m].ppm = 0.0f;
    paths[m].tx = 0;
    paths[m].reserved = 0;
    mics[m].first_path = (uint32_t)m;
    mics[m].n_paths = 1;
    mics[m].sigma = 400.0f;
    mics[m].reserved = 0;
    taps[m].delay_samples = offset[m]; /* this microphone hears the message offset[m] samples after microphone 0 */
    taps[m].weight = 1.0f / MICS;
    taps[m].mic = (uint32_t)m;
  }
  beam.first_tap = 0;
  beam.n_taps = MICS;
  rc = uc_scene_render(scene, (const uint8_t*)msg, len, &len, 1, paths, MICS, mics, MICS, dev, UC_LINK_DTYPE_F32, 78125.0, 0, n_samples, 0,
                       1, NULL);
  if (rc) {
    printf("uc_scene_render: %d (%s)\n", rc, uc_scene_last_error());
    return 1;
  }
  rc = uc_array_combine(array, dev, UC_ARRAY_DTYPE_F32, MICS, 0, n_samples, 0, taps, MICS, &beam, 1, (float*)out, 0, n_samples, 0, NULL);
  if (rc) {
    printf("uc_array_combine: %d (%s)\n", rc, uc_array_last_error());
    return 1;
  }
  if (uc_device_copy(&probe, out, sizeof(probe))) { /* joins the render and the combine */
    printf("uc_device_copy: %s\n", uc_last_error());
    return 1;
  }
  rc = uc_receive_streams(uc, out, UC_DTYPE_F32, 1, n_samples, n_samples, NULL, text, sizeof(text), &n_text, NULL, 0, NULL, NULL);
  if (rc) {
    printf("uc_receive_streams: %d (%s)\n", rc, uc_last_error());
    return 1;
  }
  text[sizeof(text) - 1] = 0;
  nl = strchr(text, '\n');
  if (nl) *nl = 0;
  printf("beam of %d microphones received \"%s\"\n", MICS, text);
  uc_device_free(0, out);
  uc_device_free(0, dev);
  uc_destroy(uc);
  uc_scene_destroy(scene);
  uc_array_destroy(array);
  return 0;
}
