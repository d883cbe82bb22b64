/* host_mic.c -- a plain C99 host of the microphone model (include/uchirp_mic.h, libuchirp_mic.so): quantises and modulates
 * silence and a full-scale tone with the library's plain-C definition (no GPU), then sends five float rows of 301 samples in
 * two calls (77 + 224 samples, the state carried on the device) through uc_mic_modulate on the GPU and compares every word
 * and the final states with uc_mic_modulate_row.  Device memory comes from libuchirp.so's helpers for hosts without the HIP
 * headers.
 * Without a GPU uc_mic_create reports the missing device and the program says so (exit code 0). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uchirp.h"
#include "uchirp_mic.h"

#define ROWS 5
#define N 301
#define CUT 77

int main(void) {
  static float x[ROWS][N];
  static int32_t q[ROWS][N], state[ROWS][4], state_gpu[ROWS][4];
  static uint32_t want[ROWS][N], got[ROWS][N];
  int32_t zeros[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st[4] = {0, 0, 0, 0};
  uint32_t words[8];
  uc_mic* mic = NULL;
  void *in = NULL, *out = NULL, *sd = NULL;
  uint32_t seed = 12345u;
  int rc, r, j, silent = 0, equal = 0, ones = 0;

  printf("uc_mic_abi_version %d (header %d)\n", uc_mic_abi_version(), UC_MIC_ABI_VERSION);
  if (uc_mic_modulate_row(zeros, 8, st, words)) {
    printf("uc_mic_modulate_row: %s\n", uc_mic_last_error());
    return 1;
  }
  for (j = 0; j < 8; j++) silent += words[j] == UC_MIC_SILENCE;
  printf("silence: %d of 8 words are 0x%08x, state %d %d %d %d\n", silent, (unsigned)UC_MIC_SILENCE, (int)st[0], (int)st[1], (int)st[2], (int)st[3]);
  if (uc_mic_quantise(zeros, 7, 1.0f, 8, q[0]) == 0) {
    printf("dtype 7 was not refused\n");
    return 1;
  }
  printf("dtype 7 refused: %s\n", uc_mic_last_error());
  /* rows of pseudo-random floats in [-1, 1) (a linear congruential generator), row 0 at DC+ full scale */
  for (r = 0; r < ROWS; r++)
    for (j = 0; j < N; j++) {
      seed = seed * 1664525u + 1013904223u;
      x[r][j] = r == 0 ? 1.0f : (float)(int32_t)seed / 2147483648.0f;
    }
  for (r = 0; r < ROWS; r++) {
    memset(state[r], 0, sizeof(state[r]));
    if (uc_mic_quantise(x[r], UC_MIC_DTYPE_F32, 8388607.0f, N, q[r]) || uc_mic_modulate_row(q[r], N, state[r], want[r])) {
      printf("host functions: %s\n", uc_mic_last_error());
      return 1;
    }
  }
  for (j = 0; j < N; j++) {
    uint32_t w = want[0][j];
    while (w) {
      ones += (int)(w & 1u);
      w >>= 1;
    }
  }
  printf("DC+ at full scale: q %d, %d ones in %d bits (three quarters: half scale)\n", (int)q[0][N - 1], ones, 32 * N);
  rc = uc_mic_create(0, 8388607.0f, &mic);
  if (rc) {
    printf("uc_mic_create: %d (%s)\n", rc, uc_mic_last_error());
    return 0;
  }
  if (uc_device_malloc(0, sizeof(x), &in) || uc_device_malloc(0, sizeof(got), &out) || uc_device_malloc(0, sizeof(state_gpu), &sd) ||
      uc_device_copy(in, x, sizeof(x)) || uc_device_copy(sd, state_gpu, sizeof(state_gpu))) { /* (static: zeros) */
    printf("allocation failed: %s\n", uc_last_error());
    return 1;
  }
  rc = uc_mic_modulate(mic, in, UC_MIC_DTYPE_F32, ROWS, CUT, N, (int32_t*)sd, (uint32_t*)out, N, NULL);
  if (rc == 0)
    rc = uc_mic_modulate(mic, (const float*)in + CUT, UC_MIC_DTYPE_F32, ROWS, N - CUT, N, (int32_t*)sd, (uint32_t*)out + CUT, N, NULL);
  if (rc) {
    printf("uc_mic_modulate: %d (%s)\n", rc, uc_mic_last_error());
    return 1;
  }
  if (uc_device_copy(got, out, sizeof(got)) || uc_device_copy(state_gpu, sd, sizeof(state_gpu))) { /* joins the calls */
    printf("uc_device_copy: %s\n", uc_last_error());
    return 1;
  }
  for (r = 0; r < ROWS; r++)
    for (j = 0; j < N; j++) equal += got[r][j] == want[r][j];
  printf("%d words in two calls, %d equal uc_mic_modulate_row's, states %s\n", ROWS * N, equal,
         memcmp(state, state_gpu, sizeof(state)) ? "differ" : "equal");
  uc_device_free(0, sd);
  uc_device_free(0, out);
  uc_device_free(0, in);
  uc_mic_destroy(mic);
  return equal == ROWS * N && !memcmp(state, state_gpu, sizeof(state)) ? 0 : 1;
}
