/* host_wcorr.c -- a plain C99 host of the band-weighted correlator (include/uchirp_wcorr.h, libuchirp_wcorr.so): renders
 * "Hello World!" for two microphones 10.25 samples apart at -12 dB (libuchirp_scene.so), correlates every window of 4
 * blocks once with weights of one and once with the weights of the chirps' band (uc_wcorr_windows on the GPU, guard 128),
 * copies the doubles to the host and prints the delay uc_wcorr_peak reads off each row.  Device memory comes from
 * libuchirp.so's helpers for hosts without the HIP headers.
 * Without a GPU uc_wcorr_create reports the missing device and the program says so (exit code 0). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uchirp.h"
#include "uchirp_wcorr.h"
#include "uchirp_scene.h"

#define MICS 2
#define BLOCK 2048
#define LEAD 30 /* blocks of noise in front */
#define BLOCKS 104
#define MAX_LAG 64
#define GUARD 128
#define LAGS (2 * MAX_LAG + 1)
#define WINDOW (4 * BLOCK)
#define WINDOWS (BLOCKS * BLOCK / WINDOW)

int main(void) {
  const char* msg = "Hello World!";
  const uint32_t len = (uint32_t)strlen(msg);
  const size_t n_samples = (size_t)BLOCKS * BLOCK;
  static const double offset[MICS] = {0.0, 10.25}; /* samples */
  static const double flat[5] = {1.0, 2.0, 3.0, 2.0, 1.0};
  static float weights[UC_WCORR_BINS];
  static double rows[2][WINDOWS][LAGS];
  uc_link_config fmt;
  uc_scene_path paths[MICS];
  uc_scene_mic mics[MICS];
  uc_wcorr_pair pair;
  uc_wcorr_peak_t peak;
  uc_scene* scene = NULL;
  uc_wcorr* wc = NULL;
  void *dev = NULL, *corr = NULL;
  double tail = 0.0;
  int rc, m, w, pass;

  printf("uc_wcorr_abi_version %d (header %d)\n", uc_wcorr_abi_version(), UC_WCORR_ABI_VERSION);
  if (uc_wcorr_band_weights(78125.0, 16000.0, 19000.0, 1000.0, GUARD, weights, &tail)) {
    printf("uc_wcorr_band_weights: %s\n", uc_wcorr_last_error());
    return 1;
  }
  printf("band 16000 .. 19000 Hz, edges 1000 Hz: w[380] %.1f, w[406] %.4f, w[446] %.1f, w[530] %.1f; tail beyond guard %d: %.2e\n", weights[380],
         weights[406], weights[446], weights[530], GUARD, tail);
  if (uc_wcorr_band_weights(78125.0, 19000.0, 16000.0, 1000.0, GUARD, weights, NULL) == 0) return 1;
  printf("f_lo > f_hi refused: %s\n", uc_wcorr_last_error());
  if (uc_wcorr_band_weights(78125.0, 16000.0, 19000.0, 1000.0, GUARD, weights, NULL)) return 1;
  if (uc_wcorr_peak(flat, 2, &peak)) {
    printf("uc_wcorr_peak: %s\n", uc_wcorr_last_error());
    return 1;
  }
  printf("crest of 1 2 3 2 1: delay %.3f, height %.3f\n", peak.delay_samples, peak.height);
  rc = uc_wcorr_create(0, &wc);
  if (rc) {
    printf("uc_wcorr_create: %d (%s)\n", rc, uc_wcorr_last_error());
    return 0;
  }
  uc_scene_default_config(&fmt);
  rc = uc_scene_create(0, &fmt, &scene);
  if (rc) {
    printf("uc_scene_create: %d (%s)\n", rc, uc_scene_last_error());
    return 1;
  }
  if (uc_device_malloc(0, MICS * n_samples * sizeof(float), &dev) || uc_device_malloc(0, sizeof(rows), &corr)) {
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
    mics[m].sigma = 7962.0f; /* -12 dB */
    mics[m].reserved = 0;
  }
  rc = uc_scene_render(scene, (const uint8_t*)msg, len, &len, 1, paths, MICS, mics, MICS, dev, UC_LINK_DTYPE_F32, 78125.0, 0, n_samples, 0,
                       1, NULL);
  if (rc) {
    printf("uc_scene_render: %d (%s)\n", rc, uc_scene_last_error());
    return 1;
  }
  pair.ref = 0;
  pair.mic = 1;
  for (pass = 0; pass < 2; pass++) { /* weights of one, then the band's */
    rc = uc_wcorr_windows(wc, dev, UC_WCORR_DTYPE_F32, MICS, n_samples, 0, &pair, 1, 0, WINDOW, WINDOW, WINDOWS, MAX_LAG, GUARD,
                          pass ? weights : NULL, (double*)corr + (size_t)pass * WINDOWS * LAGS, 0, NULL);
    if (rc) {
      printf("uc_wcorr_windows: %d (%s)\n", rc, uc_wcorr_last_error());
      return 1;
    }
  }
  if (uc_device_copy(rows, corr, sizeof(rows))) { /* joins the render and the correlator */
    printf("uc_device_copy: %s\n", uc_last_error());
    return 1;
  }
  for (w = 0; w < WINDOWS; w++) {
    uc_wcorr_peak_t plain;
    if (uc_wcorr_peak(rows[0][w], MAX_LAG, &plain) || uc_wcorr_peak(rows[1][w], MAX_LAG, &peak)) {
      printf("uc_wcorr_peak: %s\n", uc_wcorr_last_error());
      return 1;
    }
    printf("window %2d: delay %9.4f weighted, %9.4f plain (scene %.4f), runner-up %.3f, flags %u\n", w, peak.delay_samples, plain.delay_samples,
           offset[1], peak.runner_up, (unsigned)peak.flags);
  }
  uc_device_free(0, corr);
  uc_device_free(0, dev);
  uc_scene_destroy(scene);
  uc_wcorr_destroy(wc);
  return 0;
}
