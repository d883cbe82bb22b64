/* host_iir.c -- a plain C99 host of the recursive filter bank (include/uchirp_iir.h, libuchirp_iir.so): runs a one-pole
 * low-pass over a step with the library's plain-C definition (no GPU), then sends five float rows of 301 samples in two calls
 * (77 + 224 samples, the state carried on the device) through a two-section cascade with uc_iir_run on the GPU and compares
 * every output bit and the final states with uc_iir_filter_row.  Device memory comes from libuchirp.so's helpers for hosts
 * without the HIP headers.
 * Without a GPU uc_iir_create reports the missing device and the program says so (exit code 0). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uchirp.h"
#include "uchirp_iir.h"

#define ROWS 5
#define N 301
#define CUT 77

int main(void) {
  /* y[n] = 0.5 x[n] + 0.5 y[n - 1] */
  static const float one_pole[5] = {0.5f, 0.0f, 0.0f, -0.5f, 0.0f};
  /* two stable sections: a resonator at a quarter of the rate and a smoother */
  static const float cascade[10] = {0.2f, 0.0f, -0.2f, 0.0f, 0.81f, 0.25f, 0.5f, 0.25f, -0.6f, 0.2f};
  static float x[ROWS][N], want[ROWS][N], got[ROWS][N], state[ROWS][UC_IIR_STATE_WORDS], state_gpu[ROWS][UC_IIR_STATE_WORDS];
  float step[64], y[64], st[UC_IIR_STATE_WORDS];
  uc_iir* iir = NULL;
  void *in = NULL, *out = NULL, *sd = NULL;
  uint32_t seed = 12345u;
  int rc, r, j, equal = 0;

  printf("uc_iir_abi_version %d (header %d)\n", uc_iir_abi_version(), UC_IIR_ABI_VERSION);
  memset(st, 0, sizeof(st));
  for (j = 0; j < 64; j++) step[j] = 1.0f;
  if (uc_iir_filter_row(one_pole, 1, step, UC_IIR_DTYPE_F32, 64, st, y)) {
    printf("uc_iir_filter_row: %s\n", uc_iir_last_error());
    return 1;
  }
  printf("step response of the one-pole low-pass after 64 samples: %f (first %f, second %f)\n", (double)y[63], (double)y[0], (double)y[1]);
  if (uc_iir_filter_row(one_pole, 1, step, 7, 64, st, y) == 0) {
    printf("dtype 7 was not refused\n");
    return 1;
  }
  printf("dtype 7 refused: %s\n", uc_iir_last_error());
  /* rows of pseudo-random floats in [-20000, 20000) (a linear congruential generator) */
  for (r = 0; r < ROWS; r++)
    for (j = 0; j < N; j++) {
      seed = seed * 1664525u + 1013904223u;
      x[r][j] = (float)(int32_t)seed / 2147483648.0f * 20000.0f;
    }
  for (r = 0; r < ROWS; r++) {
    memset(state[r], 0, sizeof(state[r]));
    if (uc_iir_filter_row(cascade, 2, x[r], UC_IIR_DTYPE_F32, N, state[r], want[r])) {
      printf("uc_iir_filter_row: %s\n", uc_iir_last_error());
      return 1;
    }
  }
  rc = uc_iir_create(0, &iir);
  if (rc) {
    printf("uc_iir_create: %d (%s)\n", rc, uc_iir_last_error());
    return 0;
  }
  if (uc_iir_set_sections(iir, cascade, 1, 2)) {
    printf("uc_iir_set_sections: %s\n", uc_iir_last_error());
    return 1;
  }
  if (uc_device_malloc(0, sizeof(x), &in) || uc_device_malloc(0, sizeof(got), &out) || uc_device_malloc(0, sizeof(state_gpu), &sd) ||
      uc_device_copy(in, x, sizeof(x)) || uc_device_copy(sd, state_gpu, sizeof(state_gpu))) { /* (static: zeros) */
    printf("allocation failed: %s\n", uc_last_error());
    return 1;
  }
  rc = uc_iir_run(iir, in, UC_IIR_DTYPE_F32, ROWS, N, ROWS, CUT, NULL, NULL, (float*)sd, (float*)out, N, NULL);
  if (rc == 0)
    rc = uc_iir_run(iir, (const float*)in + CUT, UC_IIR_DTYPE_F32, ROWS, N, ROWS, N - CUT, NULL, NULL, (float*)sd, (float*)out + CUT, N, NULL);
  if (rc) {
    printf("uc_iir_run: %d (%s)\n", rc, uc_iir_last_error());
    return 1;
  }
  if (uc_device_copy(got, out, sizeof(got)) || uc_device_copy(state_gpu, sd, sizeof(state_gpu))) { /* joins the calls */
    printf("uc_device_copy: %s\n", uc_last_error());
    return 1;
  }
  for (r = 0; r < ROWS; r++)
    for (j = 0; j < N; j++) equal += memcmp(&got[r][j], &want[r][j], sizeof(float)) == 0;
  printf("%d samples in two calls, %d equal uc_iir_filter_row's, states %s\n", ROWS * N, equal,
         memcmp(state, state_gpu, sizeof(state)) ? "differ" : "equal");
  uc_device_free(0, sd);
  uc_device_free(0, out);
  uc_device_free(0, in);
  uc_iir_destroy(iir);
  return equal == ROWS * N && !memcmp(state, state_gpu, sizeof(state)) ? 0 : 1;
}
