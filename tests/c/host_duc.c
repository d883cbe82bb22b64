/* host_duc.c -- a plain C99 host of the up-converter (include/uchirp_duc.h, libuchirp_duc.so): interpolates a step by 4 through
 * a hold (four taps of 1) with the library's plain-C definition (no GPU), then puts four I/Q rows of 1001 samples onto four
 * carriers, two channels to each of two int16 output rows (one input row shared), interpolated by 3 through 27 taps, in two
 * calls (333 + 668 samples, the history carried on the device) with uc_duc_run on the GPU and compares every output value,
 * the clip counts and the final states with uc_duc_filter_row + uc_duc_sum_row.  Device memory comes from libuchirp.so's
 * helpers for hosts without the HIP headers.
 * Without a GPU uc_duc_create reports the missing device and the program says so (exit code 0). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uchirp.h"
#include "uchirp_duc.h"

#define IN_ROWS 4
#define ROWS 2
#define CHAN 2
#define N 1001
#define CUT 333
#define K_TAPS 9
#define INTERP 3
#define FIRST 1431655000u /* the outputs' index passes 2^32 inside the rows */
#define N_OUT (N * INTERP)

int main(void) {
  static float x[IN_ROWS][2 * N], y[ROWS * CHAN][N_OUT], state[IN_ROWS][2 * UC_DUC_STATE_SAMPLES], state_gpu[IN_ROWS][2 * UC_DUC_STATE_SAMPLES];
  static int16_t want[ROWS][N_OUT], got[ROWS][N_OUT];
  static const uint32_t row_map[ROWS * CHAN] = {0u, 1u, 1u, 3u}, steps[ROWS * CHAN] = {962072674u, 0u, 3332894622u, 2147483648u},
                        phases[ROWS * CHAN] = {0u, 0u, 77u, 4294967295u};
  uint32_t clip_want[ROWS] = {0u, 0u}, clip_got[ROWS] = {0u, 0u};
  float hold[4] = {1.0f, 1.0f, 1.0f, 1.0f}, taps[K_TAPS * INTERP], step[4] = {1.0f, 2.0f, 3.0f, 4.0f}, up[16], st[UC_DUC_STATE_SAMPLES];
  uc_duc* duc = NULL;
  void *in = NULL, *out = NULL, *sd = NULL, *cd = NULL;
  uint32_t seed = 12345u;
  int rc, r, j, equal = 0, total;

  printf("uc_duc_abi_version %d (header %d)\n", uc_duc_abi_version(), UC_DUC_ABI_VERSION);
  memset(st, 0, sizeof(st));
  if (uc_duc_filter_row(hold, 1, 4, step, UC_DUC_IN_I, 4, 0, 0, 0, st, up)) {
    printf("uc_duc_filter_row: %s\n", uc_duc_last_error());
    return 1;
  }
  printf("a step held over 4 outputs: %f %f %f %f %f ... %f (state's last %f)\n", (double)up[0], (double)up[3], (double)up[4], (double)up[7], (double)up[8],
         (double)up[15], (double)st[UC_DUC_STATE_SAMPLES - 1]);
  if (uc_duc_filter_row(hold, 1, 4, step, 7, 4, 0, 0, 0, st, up) == 0) {
    printf("format 7 was not refused\n");
    return 1;
  }
  printf("format 7 refused: %s\n", uc_duc_last_error());
  /* rows and taps of pseudo-random floats (a linear congruential generator); the rows are loud enough to clip now and then */
  for (r = 0; r < IN_ROWS; r++)
    for (j = 0; j < 2 * N; j++) {
      seed = seed * 1664525u + 1013904223u;
      x[r][j] = (float)(int32_t)seed / 2147483648.0f * 12000.0f;
    }
  for (j = 0; j < K_TAPS * INTERP; j++) {
    seed = seed * 1664525u + 1013904223u;
    taps[j] = (float)(int32_t)seed / 2147483648.0f * 0.6f;
  }
  for (r = 0; r < IN_ROWS; r++) memset(state[r], 0, sizeof(state[r]));
  for (r = 0; r < ROWS * CHAN; r++) {
    float s0[2 * UC_DUC_STATE_SAMPLES];
    memset(s0, 0, sizeof(s0));
    if (uc_duc_filter_row(taps, K_TAPS, INTERP, x[row_map[r]], UC_DUC_IN_IQ, N, FIRST, steps[r], phases[r], s0, y[r])) {
      printf("uc_duc_filter_row: %s\n", uc_duc_last_error());
      return 1;
    }
    memcpy(state[row_map[r]], s0, sizeof(s0));
  }
  for (r = 0; r < IN_ROWS; r++) { /* an input row that no channel reads still moves its state */
    float s0[2 * UC_DUC_STATE_SAMPLES], scratch[N_OUT];
    memset(s0, 0, sizeof(s0));
    if (uc_duc_filter_row(taps, K_TAPS, INTERP, x[r], UC_DUC_IN_IQ, N, FIRST, 0, 0, s0, scratch)) return 1;
    memcpy(state[r], s0, sizeof(s0));
  }
  for (r = 0; r < ROWS; r++) {
    const float* rows[CHAN];
    for (j = 0; j < CHAN; j++) rows[j] = y[r * CHAN + j];
    if (uc_duc_sum_row(rows, CHAN, N_OUT, want[r], UC_DUC_OUT_I16, &clip_want[r])) {
      printf("uc_duc_sum_row: %s\n", uc_duc_last_error());
      return 1;
    }
  }
  rc = uc_duc_create(0, &duc);
  if (rc) {
    printf("uc_duc_create: %d (%s)\n", rc, uc_duc_last_error());
    return 0;
  }
  if (uc_duc_set_taps(duc, taps, 1, K_TAPS, INTERP)) {
    printf("uc_duc_set_taps: %s\n", uc_duc_last_error());
    return 1;
  }
  if (uc_device_malloc(0, sizeof(x), &in) || uc_device_malloc(0, sizeof(got), &out) || uc_device_malloc(0, sizeof(state_gpu), &sd) ||
      uc_device_malloc(0, sizeof(clip_got), &cd) || uc_device_copy(in, x, sizeof(x)) || uc_device_copy(out, got, sizeof(got)) ||
      uc_device_copy(sd, state_gpu, sizeof(state_gpu)) || uc_device_copy(cd, clip_got, sizeof(clip_got))) { /* (static: zeros) */
    printf("allocation failed: %s\n", uc_last_error());
    return 1;
  }
  rc = uc_duc_run(duc, in, UC_DUC_IN_IQ, IN_ROWS, 2 * N, ROWS, CHAN, CUT, FIRST, row_map, NULL, steps, phases, (float*)sd, out, UC_DUC_OUT_I16, N_OUT,
                  (uint32_t*)cd, NULL);
  if (rc == 0)
    rc = uc_duc_run(duc, (const float*)in + 2 * CUT, UC_DUC_IN_IQ, IN_ROWS, 2 * N, ROWS, CHAN, N - CUT, (uint64_t)FIRST + CUT, row_map, NULL, steps, phases,
                    (float*)sd, (int16_t*)out + CUT * INTERP, UC_DUC_OUT_I16, N_OUT, (uint32_t*)cd, NULL);
  if (rc) {
    printf("uc_duc_run: %d (%s)\n", rc, uc_duc_last_error());
    return 1;
  }
  if (uc_device_copy(got, out, sizeof(got)) || uc_device_copy(state_gpu, sd, sizeof(state_gpu)) || uc_device_copy(clip_got, cd, sizeof(clip_got))) { /* joins the calls */
    printf("uc_device_copy: %s\n", uc_last_error());
    return 1;
  }
  total = ROWS * N_OUT;
  for (r = 0; r < ROWS; r++)
    for (j = 0; j < N_OUT; j++) equal += got[r][j] == want[r][j];
  printf("%d int16 values in two calls, %d equal uc_duc_filter_row + uc_duc_sum_row's, states %s, clip counts %s (%u, %u)\n", total, equal,
         memcmp(state, state_gpu, sizeof(state)) ? "differ" : "equal", memcmp(clip_want, clip_got, sizeof(clip_want)) ? "differ" : "equal",
         (unsigned)clip_got[0], (unsigned)clip_got[1]);
  uc_device_free(0, cd);
  uc_device_free(0, sd);
  uc_device_free(0, out);
  uc_device_free(0, in);
  uc_duc_destroy(duc);
  return equal == total && !memcmp(state, state_gpu, sizeof(state)) && !memcmp(clip_want, clip_got, sizeof(clip_want)) ? 0 : 1;
}
