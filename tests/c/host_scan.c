/* host_scan.c -- a plain C99 host of the beam scanner (include/uchirp_scan.h, libuchirp_scan.so): three microphones hear one
 * pseudo-random sound 0, 2.5 and 5.25 samples late under independent noise; five candidate delay vectors are scanned over two
 * windows with uc_scan_power on the GPU, every power is compared with uc_scan_power_row (the definition in plain C, no GPU)
 * bit for bit, and the best records are read: both windows name candidate 2, the one that holds the true delays.  Device
 * memory comes from libuchirp.so's helpers for hosts without the HIP headers.
 * Without a GPU uc_scan_create reports the missing device and the program says so (exit code 0). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uchirp.h"
#include "uchirp_scan.h"

#define MICS 3
#define N 1200
#define BEAMS 5
#define WINDOWS 2
#define FIRST 100
#define WLEN 500

static uint32_t seed = 12345u;

static float noise(void) {
  seed = seed * 1664525u + 1013904223u;
  return (float)(int32_t)seed / 2147483648.0f;
}

int main(void) {
  static const uint32_t mics[MICS] = {0, 1, 2};
  static const float weights[MICS] = {1.0f / 3, 1.0f / 3, 1.0f / 3};
  static const double delays[BEAMS][MICS] = {{0, 0, 0}, {0, 1.25, 2.5}, {0, 2.5, 5.25}, {0, 4.0, 8.0}, {5.25, 2.5, 0}};
  static float sound[N + 16], x[MICS][N], table[UC_SCAN_FRACTIONS * UC_SCAN_COEFS];
  double want[WINDOWS][BEAMS], got[WINDOWS][BEAMS];
  uc_scan_best best[WINDOWS];
  int32_t q[BEAMS][MICS];
  uc_scan* scan = NULL;
  void *in = NULL, *power = NULL, *rec = NULL;
  uint32_t direct = 0;
  int rc, m, j, b, w, equal = 0;

  printf("uc_scan_abi_version %d (header %d)\n", uc_scan_abi_version(), UC_SCAN_ABI_VERSION);
  if (uc_scan_table(1.0f, table) || table[7] != 1.0f || table[128 * UC_SCAN_COEFS + 7] <= 0.5f) {
    printf("uc_scan_table: %s\n", uc_scan_last_error());
    return 1;
  }
  printf("half a sample: coefficients %f %f around the centre\n", (double)table[128 * UC_SCAN_COEFS + 7], (double)table[128 * UC_SCAN_COEFS + 8]);
  /* a sound that changes slowly (a moving average of noise over four samples), delayed by linear interpolation between
   * its neighbours, plus independent noise of a tenth of its size */
  for (j = 0; j < N + 16; j++) sound[j] = 0.0f;
  for (j = 4; j < N + 16; j++) sound[j] = 2000.0f * (noise() + noise() + noise() + noise());
  for (j = N + 15; j >= 4; j--) sound[j] = 0.25f * (sound[j] + sound[j - 1] + sound[j - 2] + sound[j - 3]);
  for (j = 0; j < N; j++) {
    x[0][j] = sound[j + 8] + 100.0f * noise();
    x[1][j] = 0.5f * (sound[j + 6] + sound[j + 5]) + 100.0f * noise();                 /* 2.5 late */
    x[2][j] = 0.75f * sound[j + 3] + 0.25f * sound[j + 2] + 100.0f * noise();                                  /* 5.25 late */
  }
  for (b = 0; b < BEAMS; b++)
    for (m = 0; m < MICS; m++)
      if (uc_scan_quantise(delays[b][m], &q[b][m])) {
        printf("uc_scan_quantise: %s\n", uc_scan_last_error());
        return 1;
      }
  if (uc_scan_quantise(1e9, &q[0][0]) == 0) {
    printf("a delay of 1e9 samples was not refused\n");
    return 1;
  }
  printf("a delay of 1e9 samples refused: %s\n", uc_scan_last_error());
  for (w = 0; w < WINDOWS; w++)
    for (b = 0; b < BEAMS; b++)
      if (uc_scan_power_row(x, UC_SCAN_DTYPE_F32, MICS, 0, N, N, mics, weights, q[b], MICS, FIRST + (uint64_t)w * WLEN, WLEN, &want[w][b])) {
        printf("uc_scan_power_row: %s\n", uc_scan_last_error());
        return 1;
      }
  for (w = 0; w < WINDOWS; w++) {
    int at = 0;
    for (b = 1; b < BEAMS; b++)
      if (want[w][b] > want[w][at]) at = b;
    printf("window %d: powers %.6g %.6g %.6g %.6g %.6g, the strongest is candidate %d\n", w, want[w][0], want[w][1], want[w][2], want[w][3], want[w][4], at);
    if (at != 2) return 1;
  }
  rc = uc_scan_create(0, &scan);
  if (rc) {
    printf("uc_scan_create: %d (%s)\n", rc, uc_scan_last_error());
    return 0;
  }
  if (uc_scan_set_beams(scan, mics, weights, MICS, &delays[0][0], BEAMS, MICS) || uc_scan_direct_beams(scan, &direct)) {
    printf("uc_scan_set_beams: %s\n", uc_scan_last_error());
    return 1;
  }
  if (uc_device_malloc(0, sizeof(x), &in) || uc_device_malloc(0, sizeof(got), &power) || uc_device_malloc(0, sizeof(best), &rec) ||
      uc_device_copy(in, x, sizeof(x))) {
    printf("allocation failed: %s\n", uc_last_error());
    return 1;
  }
  rc = uc_scan_power(scan, in, UC_SCAN_DTYPE_F32, MICS, 0, N, N, 1, MICS, FIRST, WLEN, WLEN, WINDOWS, (double*)power, BEAMS, (uc_scan_best*)rec, NULL);
  if (rc) {
    printf("uc_scan_power: %d (%s)\n", rc, uc_scan_last_error());
    return 1;
  }
  if (uc_device_copy(got, power, sizeof(got)) || uc_device_copy(best, rec, sizeof(best))) { /* joins the call */
    printf("uc_device_copy: %s\n", uc_last_error());
    return 1;
  }
  for (w = 0; w < WINDOWS; w++)
    for (b = 0; b < BEAMS; b++) equal += memcmp(&got[w][b], &want[w][b], sizeof(double)) == 0;
  printf("%d powers in one call, %d equal uc_scan_power_row's; %u beams on the direct path\n", WINDOWS * BEAMS, equal, direct);
  for (w = 0; w < WINDOWS; w++) {
    printf("window %d: best beam %u, flags %u, power %.6g\n", w, best[w].beam, best[w].flags, best[w].power);
    if (best[w].beam != 2 || best[w].flags != 0 || memcmp(&best[w].power, &want[w][2], sizeof(double))) return 1;
  }
  uc_device_free(0, rec);
  uc_device_free(0, power);
  uc_device_free(0, in);
  uc_scan_destroy(scan);
  return equal == WINDOWS * BEAMS ? 0 : 1;
}
