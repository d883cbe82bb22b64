/* host_link.c -- a plain C99 host of the link simulator (include/uchirp_link.h, libuchirp_link.so): transmits
 * "Hello World!" at the WAV's own rate (44 100 Hz, int16, amplitude 20000, no noise) and prints the first samples.
 * Device memory comes from libuchirp.so's helpers for hosts without the HIP headers (uc_device_malloc / uc_device_copy).
 * Without a GPU uc_link_create reports the missing device and the program says so (exit code 0). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uchirp.h"
#include "uchirp_link.h"

int main(int argc, char** argv) {
  const char* msg = "Hello World!";
  size_t n_print = argc > 1 ? (size_t)atoi(argv[1]) : 8, n_samples = 135135, i;
  uc_link_config cfg;
  uc_link_stream p;
  uc_link* link = NULL;
  void* dev = NULL;
  int16_t* host;
  int rc;

  printf("uc_link_abi_version %d (header %d)\n", uc_link_abi_version(), UC_LINK_ABI_VERSION);
  uc_link_default_config(&cfg);
  rc = uc_link_create(0, &cfg, &link);
  if (rc) {
    printf("uc_link_create: %d (%s)\n", rc, uc_link_last_error());
    return 0;
  }
  if (n_print > n_samples) n_print = n_samples;
  host = (int16_t*)malloc(n_samples * sizeof(int16_t));
  if (!host || uc_device_malloc(0, n_samples * sizeof(int16_t), &dev)) {
    printf("allocation failed: %s\n", uc_last_error());
    return 1;
  }
  p.lead_samples = 0.0;
  p.amplitude = 20000.0f;
  p.sigma = 0.0f;
  p.ppm = 0.0f;
  p.text_len = (uint32_t)strlen(msg);
  rc = uc_link_transmit(link, (const uint8_t*)msg, strlen(msg), &p, 1, dev, UC_LINK_DTYPE_I16, 44100.0, 0, n_samples, 0, 1, NULL);
  if (rc) {
    printf("uc_link_transmit: %d (%s)\n", rc, uc_link_last_error());
    return 1;
  }
  if (uc_device_copy(host, dev, n_samples * sizeof(int16_t))) {
    printf("uc_device_copy: %s\n", uc_last_error());
    return 1;
  }
  printf("samples:");
  for (i = 0; i < n_print; ++i) printf(" %d", (int)host[1155 + i]); /* the first symbol is silence */
  printf("\n");
  uc_device_free(0, dev);
  uc_link_destroy(link);
  free(host);
  return 0;
}
