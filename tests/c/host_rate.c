/* host_rate.c -- a plain C99 host of the rate converter (include/uchirp_rate.h, libuchirp_rate.so): plans the three
 * sound-card rates and asks what one receiver block of 2048 samples needs (no GPU), then sends one int16 row at 44.1 kHz
 * that is silent but for one sample of 1000 through uc_rate_convert on the GPU: every output is then 1000 times one entry
 * of the table uc_rate_table gives, which the program checks float for float.  Device memory comes from libuchirp.so's
 * helpers for hosts without the HIP headers.
 * Without a GPU uc_rate_create reports the missing device and the program says so (exit code 0). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uchirp.h"
#include "uchirp_rate.h"

#define BLOCK 2048
#define N_IN 1764 /* one period of 3125 / 1764 */
#define AT 900    /* the sample that sounds */

int main(void) {
  static const uint32_t rates[3] = {44100, 48000, 96000};
  static int16_t pcm[N_IN];
  uc_rate_info info;
  uc_rate* cv = NULL;
  void *in = NULL, *out = NULL;
  float *table, *y;
  int64_t lo, hi, k, n_out;
  uint32_t p;
  int rc, r, equal = 0, sounding = 0;
  int64_t m;

  printf("uc_rate_abi_version %d (header %d)\n", uc_rate_abi_version(), UC_RATE_ABI_VERSION);
  for (r = 0; r < 3; r++) {
    if (uc_rate_plan(78125, rates[r], 24, 9.0, &info) || uc_rate_span(&info, 7 * BLOCK, BLOCK, &lo, &hi)) {
      printf("uc_rate_plan: %s\n", uc_rate_last_error());
      return 1;
    }
    printf("%5u Hz: %u / %u, %u taps, table of %u floats; block 7 reads input samples %lld .. %lld\n", (unsigned)rates[r], (unsigned)info.up,
           (unsigned)info.down, (unsigned)info.taps, (unsigned)info.table_len, (long long)lo, (long long)(hi - 1));
  }
  if (uc_rate_plan(5, 5, 24, 9.0, &info) == 0) {
    printf("the ratio 1 was not refused\n");
    return 1;
  }
  printf("5 / 5 refused: %s\n", uc_rate_last_error());
  rc = uc_rate_create(0, 78125, 44100, 24, 9.0, &cv);
  if (rc) {
    printf("uc_rate_create: %d (%s)\n", rc, uc_rate_last_error());
    return 0;
  }
  uc_rate_plan(78125, 44100, 24, 9.0, &info);
  n_out = uc_rate_count(&info, N_IN);
  table = (float*)malloc(info.table_len * sizeof(float));
  y = (float*)malloc((size_t)n_out * sizeof(float));
  if (!table || !y || uc_rate_table(&info, 9.0, table, info.table_len)) {
    printf("uc_rate_table: %s\n", uc_rate_last_error());
    return 1;
  }
  pcm[AT] = 1000;
  if (uc_device_malloc(0, sizeof(pcm), &in) || uc_device_malloc(0, (size_t)n_out * sizeof(float), &out) || uc_device_copy(in, pcm, sizeof(pcm))) {
    printf("allocation failed: %s\n", uc_last_error());
    return 1;
  }
  rc = uc_rate_convert(cv, in, UC_RATE_DTYPE_I16, 1, 0, N_IN, 0, (float*)out, 0, (size_t)n_out, 0, NULL);
  if (rc) {
    printf("uc_rate_convert: %d (%s)\n", rc, uc_rate_last_error());
    return 1;
  }
  if (uc_device_copy(y, out, (size_t)n_out * sizeof(float))) { /* joins the conversion */
    printf("uc_device_copy: %s\n", uc_last_error());
    return 1;
  }
  for (m = 0; m < n_out; m++) {
    float want = 0.0f;
    uc_rate_step(&info, (uint64_t)m, &k, &p);
    if (k - AT >= 0 && k - AT < (int64_t)info.taps) {
      want = table[(size_t)p * info.taps + (size_t)(k - AT)] * 1000.0f;
      sounding++;
    }
    equal += y[m] == want;
  }
  printf("%lld outputs, %d under the sample that sounds, %d equal 1000 * their table entry\n", (long long)n_out, sounding, equal);
  free(y);
  free(table);
  uc_device_free(0, out);
  uc_device_free(0, in);
  uc_rate_destroy(cv);
  return equal == n_out ? 0 : 1;
}
