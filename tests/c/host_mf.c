/* host_mf.c -- a plain C99 host of the pulse compressor (include/uchirp_mf.h, libuchirp_mf.so): plans a call, reads a
 * pulse's arrival off a crafted array with the library's host functions (no GPU), then hides a 33-tap pulse twice in two
 * float rows of 5000 noise samples, compresses them with its matched filter through uc_mf_run on the GPU, compares every
 * output with a direct sum in double inside the header's bound, and finds both arrivals in the records.  Device memory
 * comes from libuchirp.so's helpers for hosts without the HIP headers.
 * Without a GPU uc_mf_create reports the missing device and the program says so (exit code 0). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uchirp.h"
#include "uchirp_mf.h"

#define ROWS 2
#define N 5000
#define TAPS 33
#define POS0 1099511627781ull /* 2^40 + 5 */

int main(void) {
  static float x[ROWS][N], y[ROWS][2 * N];
  static uc_mf_record rec[ROWS][4];
  static const int at[ROWS][2] = {{700, 3100}, {1234, 1300}};
  float pulse[TAPS], taps[2 * TAPS], e[7] = {0.0f, 1.0f, 4.0f, 9.0f, 4.0f, 1.0f, 0.0f};
  uc_mf_job jobs[ROWS] = {{0, 0}, {1, 0}};
  uc_mf_record one;
  uc_mf* mf = NULL;
  void *in = NULL, *out = NULL, *rd = NULL;
  uint32_t seed = 2024u, hop = 0;
  uint64_t k0 = 0, ns = 0;
  double off = 0.0, top = 0.0, worst = 0.0, hnorm = 0.0, xnorm;
  int rc, r, j, k, found = 0;

  printf("uc_mf_abi_version %d (header %d)\n", uc_mf_abi_version(), UC_MF_ABI_VERSION);
  if (uc_mf_plan(TAPS, POS0, 0, N, &hop, &k0, &ns) || hop != 2048 - TAPS - 1 || ns > 4) {
    printf("uc_mf_plan: %s\n", uc_mf_last_error());
    return 1;
  }
  printf("plan: hop %u, segments %llu .. %llu\n", hop, (unsigned long long)k0, (unsigned long long)(k0 + ns - 1));
  if (uc_mf_select(e, 5, 0, 5, &one) || one.n_cand != 1 || one.cand[0].offset != 2 || uc_mf_arrival(&one.cand[0], &off, &top) || off != 2.0 ||
      top != 3.0) {
    printf("uc_mf_select / uc_mf_arrival: %s\n", uc_mf_last_error());
    return 1;
  }
  printf("a crest of height %g at offset %g\n", top, off);
  if (uc_mf_plan(0, 0, 0, 1, &hop, &k0, &ns) == 0) {
    printf("0 taps were not refused\n");
    return 1;
  }
  printf("0 taps refused: %s\n", uc_mf_last_error());
  if (uc_mf_plan(TAPS, POS0, 0, N, &hop, &k0, &ns)) return 1;
  /* a pulse of pseudo-random signs (a linear congruential generator), twice in every row of noise; its matched filter */
  for (j = 0; j < TAPS; j++) {
    seed = seed * 1664525u + 1013904223u;
    pulse[j] = (seed >> 31) ? 100.0f : -100.0f;
  }
  for (j = 0; j < TAPS; j++) {
    taps[2 * j] = pulse[TAPS - 1 - j] / 100.0f;
    taps[2 * j + 1] = 0.0f;
    hnorm += 1.0;
  }
  hnorm = sqrt(hnorm);
  for (r = 0; r < ROWS; r++) {
    for (j = 0; j < N; j++) {
      seed = seed * 1664525u + 1013904223u;
      x[r][j] = (float)(int32_t)seed / 2147483648.0f * 20.0f;
    }
    for (k = 0; k < 2; k++)
      for (j = 0; j < TAPS; j++) x[r][at[r][k] + j] += pulse[j];
  }
  rc = uc_mf_create(0, &mf);
  if (rc) {
    printf("uc_mf_create: %d (%s)\n", rc, uc_mf_last_error());
    return 0;
  }
  if (uc_mf_set_templates(mf, taps, 1, TAPS)) {
    printf("uc_mf_set_templates: %s\n", uc_mf_last_error());
    return 1;
  }
  if (uc_device_malloc(0, sizeof(x), &in) || uc_device_malloc(0, sizeof(y), &out) || uc_device_malloc(0, sizeof(rec), &rd) ||
      uc_device_copy(in, x, sizeof(x))) {
    printf("allocation failed: %s\n", uc_last_error());
    return 1;
  }
  rc = uc_mf_run(mf, in, UC_MF_DTYPE_F32, ROWS, N, 0, jobs, ROWS, POS0, 0, N, out, UC_MF_OUT_COMPLEX, 0, (uc_mf_record*)rd, NULL);
  if (rc) {
    printf("uc_mf_run: %d (%s)\n", rc, uc_mf_last_error());
    return 1;
  }
  if (uc_device_copy(y, out, sizeof(y)) || uc_device_copy(rec, rd, (size_t)ROWS * ns * sizeof(uc_mf_record))) { /* joins the call */
    printf("uc_device_copy: %s\n", uc_last_error());
    return 1;
  }
  /* every output against the direct sum; ||a_k|| <= the norm of the whole row */
  for (r = 0; r < ROWS; r++) {
    xnorm = 0.0;
    for (j = 0; j < N; j++) xnorm += (double)x[r][j] * x[r][j];
    xnorm = sqrt(xnorm);
    for (j = 0; j < N; j++) {
      double s = 0.0, d;
      for (k = 0; k < TAPS && k <= j; k++) s += (double)taps[2 * k] * x[r][j - k];
      d = fabs(y[r][2 * j] - s) + fabs(y[r][2 * j + 1]);
      if (d / (xnorm * hnorm) > worst) worst = d / (xnorm * hnorm);
    }
  }
  /* records are laid out [job][segment]; an arrival at sample p peaks at output p + TAPS - 1 */
  for (r = 0; r < ROWS; r++)
    for (k = 0; k < 2; k++) {
      const uint64_t q = POS0 + (uint64_t)at[r][k] + TAPS - 1;
      const uc_mf_record* rr = (const uc_mf_record*)rec + (size_t)r * ns + (q / hop - k0);
      for (j = 0; j < UC_MF_CANDIDATES; j++)
        if (rr->cand[j].peak > 0.0f && (q / hop) * hop + rr->cand[j].offset == q && rr->cand[j].peak > 0.5f * 3300.0f * 3300.0f) found++;
    }
  printf("%d outputs, worst error %.3g of 2^-24 ||x|| ||h|| (bound %d), %d of 4 arrivals in the records\n", ROWS * N, worst * 16777216.0,
         UC_MF_ERROR_C, found);
  uc_device_free(0, rd);
  uc_device_free(0, out);
  uc_device_free(0, in);
  uc_mf_destroy(mf);
  return worst * 16777216.0 <= UC_MF_ERROR_C && found == 4 ? 0 : 1;
}
