/* host_track.c -- a plain C99 host of the delay tracker (include/uchirp_track.h, libuchirp_track.so): renders
 * "Hello World!" for two microphones 97.5 samples apart (libuchirp_scene.so), asks for the crest records of every window of
 * 4 blocks in ONE call (uc_track_windows on the GPU), copies the records (136 bytes each) to the host and prints the
 * delay uc_track_finish reads off each of them.  Device memory comes from libuchirp.so's helpers for hosts without the HIP
 * headers.
 * Without a GPU uc_track_create reports the missing device and the program says so (exit code 0). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uchirp.h"
#include "uchirp_track.h"
#include "uchirp_scene.h"

#define MICS 2
#define BLOCK 2048
#define LEAD 30 /* blocks of noise in front */
#define BLOCKS 104
#define MAX_LAG 128
#define WINDOW (4 * BLOCK)
#define WINDOWS (BLOCKS * BLOCK / WINDOW)

int main(void) {
  const char* msg = "Hello World!";
  const uint32_t len = (uint32_t)strlen(msg);
  const size_t n_samples = (size_t)BLOCKS * BLOCK;
  static const double offset[MICS] = {0.0, 97.5}; /* samples */
  uc_link_config fmt;
  uc_scene_path paths[MICS];
  uc_scene_mic mics[MICS];
  uc_track_pair pair;
  uc_track_peak_t peak;
  uc_track_crest flat;
  uc_scene* scene = NULL;
  uc_track* tr = NULL;
  void *dev = NULL, *crest = NULL;
  static uc_track_crest rec[WINDOWS];
  int rc, m, w;

  printf("uc_track_abi_version %d (header %d)\n", uc_track_abi_version(), UC_TRACK_ABI_VERSION);
  memset(&flat, 0, sizeof(flat));
  flat.n_candidates = 1;
  flat.slot[0].k = 2;
  flat.slot[0].r[0] = 2.0;
  flat.slot[0].r[1] = 3.0;
  flat.slot[0].r[2] = 2.0;
  for (m = 1; m < UC_TRACK_SLOTS; m++) flat.slot[m].k = -1;
  if (uc_track_finish(&flat, 2, &peak)) {
    printf("uc_track_finish: %s\n", uc_track_last_error());
    return 1;
  }
  printf("crest 2 3 2 at k = 2 of 1 2 3 2 1: delay %.3f, height %.3f\n", peak.delay_samples, peak.height);
  rc = uc_track_create(0, &tr);
  if (rc) {
    printf("uc_track_create: %d (%s)\n", rc, uc_track_last_error());
    return 0;
  }
  uc_scene_default_config(&fmt);
  rc = uc_scene_create(0, &fmt, &scene);
  if (rc) {
    printf("uc_scene_create: %d (%s)\n", rc, uc_scene_last_error());
    return 1;
  }
  if (uc_device_malloc(0, MICS * n_samples * sizeof(float), &dev) || uc_device_malloc(0, sizeof(rec), &crest)) {
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
  pair.ref = 0;
  pair.mic = 1;
  rc = uc_track_windows(tr, dev, UC_TRACK_DTYPE_F32, MICS, n_samples, 0, &pair, 1, 0, WINDOW, WINDOW, WINDOWS, MAX_LAG, NULL, 0,
                        (uc_track_crest*)crest, NULL);
  if (rc) {
    printf("uc_track_windows: %d (%s)\n", rc, uc_track_last_error());
    return 1;
  }
  if (uc_device_copy(rec, crest, sizeof(rec))) { /* joins the render and the tracker */
    printf("uc_device_copy: %s\n", uc_last_error());
    return 1;
  }
  for (w = 0; w < WINDOWS; w++) {
    if (uc_track_finish(&rec[w], MAX_LAG, &peak)) {
      printf("uc_track_finish: %s\n", uc_track_last_error());
      return 1;
    }
    printf("window %2d: delay %9.4f (scene %.4f), height %.4g, runner-up %.3f, candidates %u, flags %u\n", w, peak.delay_samples, offset[1],
           peak.height, peak.runner_up, (unsigned)rec[w].n_candidates, (unsigned)peak.flags);
  }
  uc_device_free(0, crest);
  uc_device_free(0, dev);
  uc_scene_destroy(scene);
  uc_track_destroy(tr);
  return 0;
}
