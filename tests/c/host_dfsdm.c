/* host_dfsdm.c -- a plain C99 host of the DFSDM filter (include/uchirp_dfsdm.h, libuchirp_dfsdm.so): checks, plans and
 * filters with the library's host functions (no GPU), then sends five rows of 67 words in two calls (17 + 50 words, the
 * state carried on the device, words_before advanced) through uc_dfsdm_run on the GPU, at SINC3 / 32 (the word path) and at
 * FastSinc / 20 (the bit path), and compares every word and the final states with uc_dfsdm_filter_row.  Device memory comes
 * from libuchirp.so's helpers for hosts without the HIP headers.
 * Without a GPU uc_dfsdm_create reports the missing device and the program says so (exit code 0). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uchirp.h"
#include "uchirp_dfsdm.h"

#define ROWS 5
#define N 67
#define CUT 17
#define CAP (32 * N)

int main(void) {
  static uint32_t pdm[ROWS][N], silent[N];
  static int32_t want[ROWS][CAP], got[ROWS][CAP], state[ROWS][16], state_gpu[ROWS][16], row[CAP];
  const uc_dfsdm_config configs[2] = {{3, 32, 1, 2, 0}, {UC_DFSDM_ORDER_FASTSINC, 20, 1, 0, 0}};
  uc_dfsdm_config bad = {5, 74, 1, 0, 0};
  int32_t st[16];
  uint64_t planned = 0, first = 0, second = 0;
  size_t n_out = 0;
  uint32_t seed = 12345u;
  void *in = NULL, *out = NULL, *sd = NULL;
  int rc, r, j, c, zero = 0;

  printf("uc_dfsdm_abi_version %d (header %d)\n", uc_dfsdm_abi_version(), UC_DFSDM_ABI_VERSION);
  if (uc_dfsdm_check(&configs[0]) || uc_dfsdm_check(&configs[1])) {
    printf("uc_dfsdm_check: %s\n", uc_dfsdm_last_error());
    return 1;
  }
  printf("SINC3 / 32: gain %llu\n", (unsigned long long)uc_dfsdm_gain(&configs[0]));
  if (uc_dfsdm_check(&bad) == 0) {
    printf("sinc5 ratio 74 was not refused\n");
    return 1;
  }
  printf("sinc5 ratio 74 refused: %s\n", uc_dfsdm_last_error());
  for (j = 0; j < N; j++) silent[j] = 0x99999999u;
  memset(st, 0, sizeof(st));
  if (uc_dfsdm_filter_row(&configs[0], silent, N, 0, st, row, CAP, &n_out) || n_out != N) {
    printf("uc_dfsdm_filter_row: %s\n", uc_dfsdm_last_error());
    return 1;
  }
  for (j = 3; j < N; j++) zero += row[j] == 0;
  printf("silence: %d of %d words behind the fill are 0\n", zero, N - 3);
  /* rows of pseudo-random words (a linear congruential generator, its high bits) */
  for (r = 0; r < ROWS; r++)
    for (j = 0; j < N; j++) {
      seed = seed * 1664525u + 1013904223u;
      pdm[r][j] = seed ^ (seed >> 16);
    }
  rc = 0;
  for (c = 0; c < 2 && rc == 0; c++) {
    const uc_dfsdm_config* cfg = &configs[c];
    uc_dfsdm* obj = NULL;
    int equal = 0;
    if (uc_dfsdm_plan(cfg, 0, N, &planned) || uc_dfsdm_plan(cfg, 0, CUT, &first) || uc_dfsdm_plan(cfg, CUT, N - CUT, &second) ||
        first + second != planned) {
      printf("uc_dfsdm_plan: %llu + %llu != %llu (%s)\n", (unsigned long long)first, (unsigned long long)second, (unsigned long long)planned,
             uc_dfsdm_last_error());
      return 1;
    }
    for (r = 0; r < ROWS; r++) {
      memset(state[r], 0, sizeof(state[r]));
      if (uc_dfsdm_filter_row(cfg, pdm[r], N, 0, state[r], want[r], CAP, &n_out) || n_out != planned) {
        printf("uc_dfsdm_filter_row: %s\n", uc_dfsdm_last_error());
        return 1;
      }
    }
    printf("order %d ratio %u: %llu words per row (%llu + %llu)\n", (int)cfg->order, (unsigned)cfg->ratio, (unsigned long long)planned,
           (unsigned long long)first, (unsigned long long)second);
    rc = uc_dfsdm_create(0, cfg, &obj);
    if (rc) {
      printf("uc_dfsdm_create: %d (%s)\n", rc, uc_dfsdm_last_error());
      return 0;
    }
    memset(state_gpu, 0, sizeof(state_gpu));
    memset(got, 0, sizeof(got));
    if (uc_device_malloc(0, sizeof(pdm), &in) || uc_device_malloc(0, sizeof(got), &out) || uc_device_malloc(0, sizeof(state_gpu), &sd) ||
        uc_device_copy(in, pdm, sizeof(pdm)) || uc_device_copy(sd, state_gpu, sizeof(state_gpu)) || uc_device_copy(out, got, sizeof(got))) {
      printf("allocation failed: %s\n", uc_last_error());
      return 1;
    }
    rc = uc_dfsdm_run(obj, (const uint32_t*)in, ROWS, CUT, N, 0, (int32_t*)sd, (int32_t*)out, CAP, NULL);
    if (rc == 0)
      rc = uc_dfsdm_run(obj, (const uint32_t*)in + CUT, ROWS, N - CUT, N, CUT, (int32_t*)sd, (int32_t*)out + first, CAP, NULL);
    if (rc) {
      printf("uc_dfsdm_run: %d (%s)\n", rc, uc_dfsdm_last_error());
      return 1;
    }
    if (uc_device_copy(got, out, sizeof(got)) || uc_device_copy(state_gpu, sd, sizeof(state_gpu))) { /* joins the calls */
      printf("uc_device_copy: %s\n", uc_last_error());
      return 1;
    }
    for (r = 0; r < ROWS; r++)
      for (j = 0; j < (int)planned; j++) equal += got[r][j] == want[r][j];
    printf("order %d ratio %u: %d words in two calls, %d equal uc_dfsdm_filter_row's, states %s\n", (int)cfg->order, (unsigned)cfg->ratio,
           ROWS * (int)planned, equal, memcmp(state, state_gpu, sizeof(state)) ? "differ" : "equal");
    if (equal != ROWS * (int)planned || memcmp(state, state_gpu, sizeof(state))) rc = 1;
    uc_device_free(0, sd);
    uc_device_free(0, out);
    uc_device_free(0, in);
    uc_dfsdm_destroy(obj);
  }
  return rc;
}
