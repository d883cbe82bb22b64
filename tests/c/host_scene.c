/* host_scene.c -- a plain C99 host of the scene renderer (include/uchirp_scene.h, libuchirp_scene.so): renders
 * "Hello World!" with one echo (gain 0.3, a different delay per microphone) and noise for 4 microphones, as float at
 * 78 125 Hz, and prints what uc_receive_streams (libuchirp.so, the complex-reference receiver) decodes from the device
 * buffer.  Device memory comes from libuchirp.so's helpers for hosts without the HIP headers.
 * Without a GPU uc_scene_create reports the missing device and the program says so (exit code 0). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uchirp.h"
#include "uchirp_scene.h"

#define MICS 4
#define BLOCK 2048
#define LEAD 30 /* blocks of noise in front: the receiver's mag_mean needs 24 of them */
#define BLOCKS 160

int main(void) {
  const char* msg = "Hello World!";
  const uint32_t len = (uint32_t)strlen(msg);
  const size_t n_samples = (size_t)BLOCKS * BLOCK;
  static const double delay[MICS] = {40.0, 78.125, 160.5, 240.0}; /* samples: 0.5 .. 3 ms */
  uc_link_config fmt;
  uc_scene_path paths[2 * MICS];
  uc_scene_mic mics[MICS];
  uc_scene* scene = NULL;
  uc_config cfg;
  uc_ctx* uc = NULL;
  void* dev = NULL;
  char text[MICS][64];
  uint32_t n_text[MICS];
  float probe;
  int rc, m;

  printf("uc_scene_abi_version %d (header %d)\n", uc_scene_abi_version(), UC_SCENE_ABI_VERSION);
  uc_scene_default_config(&fmt);
  rc = uc_scene_create(0, &fmt, &scene);
  if (rc) {
    printf("uc_scene_create: %d (%s)\n", rc, uc_scene_last_error());
    return 0;
  }
  if (uc_default_config(UC_SYNC_CPLX, &cfg) != 0 || uc_create(&cfg, &uc) != 0) {
    printf("uc_create: %s\n", uc_last_error());
    return 1;
  }
  if (uc_device_malloc(0, MICS * n_samples * sizeof(float), &dev)) {
    printf("allocation failed: %s\n", uc_last_error());
    return 1;
  }
  for (m = 0; m < MICS; m++) {
    uc_scene_path* p = paths + 2 * m;
    p[0].lead_samples = (double)LEAD * BLOCK + 100.25 * m;
    p[0].gain = 2000.0f;
    p[0].ppm = 0.0f;
    p[0].tx = 0;
    p[0].reserved = 0;
    p[1] = p[0];
    p[1].lead_samples += delay[m];
    p[1].gain = 0.3f * 2000.0f;
    mics[m].first_path = (uint32_t)(2 * m);
    mics[m].n_paths = 2;
    mics[m].sigma = 50.0f;
    mics[m].reserved = 0;
  }
  rc = uc_scene_render(scene, (const uint8_t*)msg, len, &len, 1, paths, 2 * MICS, mics, MICS, dev, UC_LINK_DTYPE_F32, 78125.0, 0,
                       n_samples, 0, 1, NULL);
  if (rc) {
    printf("uc_scene_render: %d (%s)\n", rc, uc_scene_last_error());
    return 1;
  }
  if (uc_device_copy(&probe, dev, sizeof(probe))) { /* joins the render */
    printf("uc_device_copy: %s\n", uc_last_error());
    return 1;
  }
  rc = uc_receive_streams(uc, dev, UC_DTYPE_F32, MICS, n_samples, n_samples, NULL, &text[0][0], sizeof(text[0]), n_text, NULL, 0, NULL,
                          NULL);
  if (rc) {
    printf("uc_receive_streams: %d (%s)\n", rc, uc_last_error());
    return 1;
  }
  for (m = 0; m < MICS; m++) {
    char* nl;
    text[m][sizeof(text[0]) - 1] = 0;
    nl = strchr(text[m], '\n');
    if (nl) *nl = 0;
    printf("microphone %d (echo %.3f samples late) received \"%s\"\n", m, delay[m], text[m]);
  }
  uc_device_free(0, dev);
  uc_destroy(uc);
  uc_scene_destroy(scene);
  return 0;
}
