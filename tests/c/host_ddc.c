/* host_ddc.c -- a plain C99 host of the down-converter (include/uchirp_ddc.h, libuchirp_ddc.so): runs an 8-tap moving average
 * over a step with the library's plain-C definition (no GPU), then converts five float rows of 1001 samples at five carriers in
 * two calls (333 + 668 samples, the history carried on the device) through 27 taps, decimated by 3, with uc_ddc_run on the GPU
 * and compares every output bit and the final states with uc_ddc_filter_row.  Device memory comes from libuchirp.so's helpers
 * for hosts without the HIP headers.
 * Without a GPU uc_ddc_create reports the missing device and the program says so (exit code 0). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uchirp.h"
#include "uchirp_ddc.h"

#define ROWS 5
#define N 1001
#define CUT 333
#define TAPS 27
#define DECIM 3
#define FIRST 4294966000u /* the phase's index wraps inside the rows */
#define MAX_OUT (2 * (N / DECIM + 2))

int main(void) {
  static float x[ROWS][N], want[ROWS][MAX_OUT], got[ROWS][MAX_OUT], state[ROWS][UC_DDC_STATE_WORDS], state_gpu[ROWS][UC_DDC_STATE_WORDS];
  static const uint32_t steps[ROWS] = {962072674u, 0u, 3332894622u, 1u, 2147483648u}, phases[ROWS] = {0u, 0u, 77u, 4294967295u, 1073741824u};
  float average[8], taps[TAPS], step[16], y[16], st[UC_DDC_STATE_WORDS];
  uc_ddc* ddc = NULL;
  void *in = NULL, *out = NULL, *sd = NULL;
  uint32_t seed = 12345u;
  uint64_t p_first = 0, p_cut = 0;
  size_t count = 0, count_a = 0, count_b = 0;
  int rc, r, j, equal = 0, total;

  printf("uc_ddc_abi_version %d (header %d)\n", uc_ddc_abi_version(), UC_DDC_ABI_VERSION);
  memset(st, 0, sizeof(st));
  for (j = 0; j < 8; j++) average[j] = 0.125f;
  for (j = 0; j < 16; j++) step[j] = 1.0f;
  if (uc_ddc_filter_row(average, 8, 1, step, UC_DDC_DTYPE_F32, 16, 0, 0, 0, st, y, UC_DDC_OUT_I)) {
    printf("uc_ddc_filter_row: %s\n", uc_ddc_last_error());
    return 1;
  }
  printf("moving average of a step after 8 samples: %f (first %f, second %f)\n", (double)y[7], (double)y[0], (double)y[1]);
  if (uc_ddc_filter_row(average, 8, 1, step, 7, 16, 0, 0, 0, st, y, UC_DDC_OUT_I) == 0) {
    printf("dtype 7 was not refused\n");
    return 1;
  }
  printf("dtype 7 refused: %s\n", uc_ddc_last_error());
  /* rows and taps of pseudo-random floats (a linear congruential generator) */
  for (r = 0; r < ROWS; r++)
    for (j = 0; j < N; j++) {
      seed = seed * 1664525u + 1013904223u;
      x[r][j] = (float)(int32_t)seed / 2147483648.0f * 20000.0f;
    }
  for (j = 0; j < TAPS; j++) {
    seed = seed * 1664525u + 1013904223u;
    taps[j] = (float)(int32_t)seed / 2147483648.0f * 0.2f;
  }
  if (uc_ddc_outputs(FIRST, N, DECIM, &p_first, &count) || uc_ddc_outputs(FIRST, CUT, DECIM, &p_first, &count_a) ||
      uc_ddc_outputs((uint64_t)FIRST + CUT, N - CUT, DECIM, &p_cut, &count_b) || count != count_a + count_b || p_cut != p_first + count_a ||
      2 * count > MAX_OUT) {
    printf("uc_ddc_outputs: %s (%lu = %lu + %lu?)\n", uc_ddc_last_error(), (unsigned long)count, (unsigned long)count_a, (unsigned long)count_b);
    return 1;
  }
  for (r = 0; r < ROWS; r++) {
    memset(state[r], 0, sizeof(state[r]));
    if (uc_ddc_filter_row(taps, TAPS, DECIM, x[r], UC_DDC_DTYPE_F32, N, FIRST, steps[r], phases[r], state[r], want[r], UC_DDC_OUT_IQ)) {
      printf("uc_ddc_filter_row: %s\n", uc_ddc_last_error());
      return 1;
    }
  }
  rc = uc_ddc_create(0, &ddc);
  if (rc) {
    printf("uc_ddc_create: %d (%s)\n", rc, uc_ddc_last_error());
    return 0;
  }
  if (uc_ddc_set_taps(ddc, taps, 1, TAPS, DECIM)) {
    printf("uc_ddc_set_taps: %s\n", uc_ddc_last_error());
    return 1;
  }
  if (uc_device_malloc(0, sizeof(x), &in) || uc_device_malloc(0, sizeof(got), &out) || uc_device_malloc(0, sizeof(state_gpu), &sd) ||
      uc_device_copy(in, x, sizeof(x)) || uc_device_copy(out, got, sizeof(got)) || uc_device_copy(sd, state_gpu, sizeof(state_gpu))) { /* (static: zeros) */
    printf("allocation failed: %s\n", uc_last_error());
    return 1;
  }
  rc = uc_ddc_run(ddc, in, UC_DDC_DTYPE_F32, ROWS, N, ROWS, CUT, FIRST, NULL, NULL, steps, phases, (float*)sd, (float*)out, UC_DDC_OUT_IQ, MAX_OUT, NULL);
  if (rc == 0)
    rc = uc_ddc_run(ddc, (const float*)in + CUT, UC_DDC_DTYPE_F32, ROWS, N, ROWS, N - CUT, (uint64_t)FIRST + CUT, NULL, NULL, steps, phases, (float*)sd,
                    (float*)out + 2 * count_a, UC_DDC_OUT_IQ, MAX_OUT, NULL);
  if (rc) {
    printf("uc_ddc_run: %d (%s)\n", rc, uc_ddc_last_error());
    return 1;
  }
  if (uc_device_copy(got, out, sizeof(got)) || uc_device_copy(state_gpu, sd, sizeof(state_gpu))) { /* joins the calls */
    printf("uc_device_copy: %s\n", uc_last_error());
    return 1;
  }
  total = ROWS * 2 * (int)count;
  for (r = 0; r < ROWS; r++)
    for (j = 0; j < 2 * (int)count; j++) equal += memcmp(&got[r][j], &want[r][j], sizeof(float)) == 0;
  printf("%d floats in two calls, %d equal uc_ddc_filter_row's, states %s\n", total, equal, memcmp(state, state_gpu, sizeof(state)) ? "differ" : "equal");
  uc_device_free(0, sd);
  uc_device_free(0, out);
  uc_device_free(0, in);
  uc_ddc_destroy(ddc);
  return equal == total && !memcmp(state, state_gpu, sizeof(state)) ? 0 : 1;
}
