/* host_xcorr.c -- a plain C99 host of the wide-lag correlator (include/uchirp_xcorr.h, libuchirp_xcorr.so): renders
 * "Hello World!" for an array of 4 microphones, each at its own fractional lead and with its own noise
 * (libuchirp_scene.so; the leads differ by hundreds of samples), ESTIMATES the delays of microphones 1 .. 3 against microphone 0 (uc_xcorr_correlate on the GPU,
 * uc_xcorr_peak on the host), steers one delay-and-sum beam with the estimates (libuchirp_array.so), and prints what
 * uc_receive_streams (libuchirp.so, the complex-reference receiver) decodes from the beam.  Device memory comes from
 * libuchirp.so's helpers for hosts without the HIP headers.
 * Without a GPU uc_xcorr_create reports the missing device and the program says so (exit code 0). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uchirp.h"
#include "uchirp_xcorr.h"
#include "uchirp_array.h"
#include "uchirp_scene.h"

#define MICS 4
#define BLOCK 2048
#define LEAD 30 /* blocks of noise in front: the receiver's mag_mean needs 24 of them */
#define BLOCKS 160
#define MAX_LAG 512
#define LAGS (2 * MAX_LAG + 1)

int main(void) {
  const char* msg = "Hello World!";
  const uint32_t len = (uint32_t)strlen(msg);
  const size_t n_samples = (size_t)BLOCKS * BLOCK;
  static const double offset[MICS] = {0.0, 97.5, 311.25, 460.375}; /* samples */
  static const double flat[5] = {1.0, 2.0, 3.0, 2.0, 1.0};
  uc_link_config fmt;
  uc_scene_path paths[MICS];
  uc_scene_mic mics[MICS];
  uc_xcorr_pair pairs[MICS - 1];
  uc_xcorr_peak_t peak;
  uc_array_tap taps[MICS];
  uc_array_beam beam;
  uc_scene* scene = NULL;
  uc_xcorr* xc = NULL;
  uc_array* array = NULL;
  uc_config cfg;
  uc_ctx* uc = NULL;
  void *dev = NULL, *out = NULL, *corr = NULL;
  static double rows[(MICS - 1) * LAGS];
  char text[64];
  uint32_t n_text;
  char* nl;
  int rc, m;

  printf("uc_xcorr_abi_version %d (header %d)\n", uc_xcorr_abi_version(), UC_XCORR_ABI_VERSION);
  if (uc_xcorr_peak(flat, 2, &peak)) {
    printf("uc_xcorr_peak: %s\n", uc_xcorr_last_error());
    return 1;
  }
  printf("peak of 1 2 3 2 1: delay %.3f, height %.3f\n", peak.delay_samples, peak.height);
  rc = uc_xcorr_create(0, &xc);
  if (rc) {
    printf("uc_xcorr_create: %d (%s)\n", rc, uc_xcorr_last_error());
    return 0;
  }
  rc = uc_array_create(0, &array);
  if (rc) {
    printf("uc_array_create: %d (%s)\n", rc, uc_array_last_error());
    return 1;
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
  if (uc_device_malloc(0, MICS * n_samples * sizeof(float), &dev) || uc_device_malloc(0, n_samples * sizeof(float), &out) ||
      uc_device_malloc(0, sizeof(rows), &corr)) {
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
  }
  rc = uc_scene_render(scene, (const uint8_t*)msg, len, &len, 1, paths, MICS, mics, MICS, dev, UC_LINK_DTYPE_F32, 78125.0, 0, n_samples, 0,
                       1, NULL);
  if (rc) {
    printf("uc_scene_render: %d (%s)\n", rc, uc_scene_last_error());
    return 1;
  }
  for (m = 1; m < MICS; m++) {
    pairs[m - 1].ref = 0;
    pairs[m - 1].mic = (uint32_t)m;
  }
  rc = uc_xcorr_correlate(xc, dev, UC_XCORR_DTYPE_F32, MICS, n_samples, 0, pairs, MICS - 1, 0, n_samples, MAX_LAG, (double*)corr, 0, NULL);
  if (rc) {
    printf("uc_xcorr_correlate: %d (%s)\n", rc, uc_xcorr_last_error());
    return 1;
  }
  if (uc_device_copy(rows, corr, sizeof(rows))) { /* joins the render and the correlation */
    printf("uc_device_copy: %s\n", uc_last_error());
    return 1;
  }
  taps[0].delay_samples = 0.0;
  for (m = 1; m < MICS; m++) {
    if (uc_xcorr_peak(rows + (size_t)(m - 1) * LAGS, MAX_LAG, &peak)) {
      printf("uc_xcorr_peak: %s\n", uc_xcorr_last_error());
      return 1;
    }
    printf("microphone %d: estimated delay %.4f (scene %.4f), runner-up %.3f, flags %u\n", m, peak.delay_samples, offset[m], peak.runner_up,
           (unsigned)peak.flags);
    taps[m].delay_samples = peak.delay_samples;
  }
  for (m = 0; m < MICS; m++) {
    taps[m].weight = 1.0f / MICS;
    taps[m].mic = (uint32_t)m;
  }
  beam.first_tap = 0;
  beam.n_taps = MICS;
  rc = uc_array_combine(array, dev, UC_ARRAY_DTYPE_F32, MICS, 0, n_samples, 0, taps, MICS, &beam, 1, (float*)out, 0, n_samples, 0, NULL);
  if (rc) {
    printf("uc_array_combine: %d (%s)\n", rc, uc_array_last_error());
    return 1;
  }
  if (uc_device_copy(rows, out, sizeof(float))) { /* joins the combine */
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
  printf("beam of %d microphones steered by estimated delays received \"%s\"\n", MICS, text);
  uc_device_free(0, corr);
  uc_device_free(0, out);
  uc_device_free(0, dev);
  uc_destroy(uc);
  uc_scene_destroy(scene);
  uc_array_destroy(array);
  uc_xcorr_destroy(xc);
  return 0;
}
