// san_xcorr.cpp -- a stand-alone driver of the host translation unit of libuchirp_xcorr.so (csrc/uc_xcorr_api.cpp) for
// tools/sanitize.sh: the peak rule over random, tied, flat and non-finite rows of every length, the errors of the entry
// points that need no GPU, and -- where a GPU is missing, as in the sanitizer's container -- the refusal of
// uc_xcorr_create.  CPU only: it never launches a kernel.
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "uchirp_xcorr.h"

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      printf("san_xcorr: %s failed (line %d)\n", #c, __LINE__);      \
      return 1;                                                      \
    }                                                                \
  } while (0)

int main() {
  std::mt19937_64 rng(9);
  std::normal_distribution<double> g(0.0, 1.0);
  uc_xcorr_peak_t out;
  int rows = 0;
  for (uint32_t L = 1; L <= UC_XCORR_MAX_LAG; L += (L < 70 ? 1 : 37)) {
    std::vector<double> r(2 * L + 1);   // exactly the row: a read past it is a report
    for (int kind = 0; kind < 4; ++kind) {
      for (double& v : r) v = kind == 0 ? g(rng) * 1e9 : kind == 1 ? std::round(g(rng) * 2.0) : kind == 2 ? 1.0 : -std::fabs(g(rng));
      CHECK(uc_xcorr_peak(r.data(), L, &out) == 0);
      CHECK(out.lag >= -(int32_t)L && out.lag <= (int32_t)L && std::isfinite(out.delay_samples) && out.runner_up >= 0.0 && out.runner_up <= 1.0);
      CHECK((out.flags & UC_XCORR_NO_PEAK) == 0 || (out.height == 0.0 && out.lag == 0));
      ++rows;
    }
    r[2 * L] = NAN;
    CHECK(uc_xcorr_peak(r.data(), L, &out) == -EINVAL && strlen(uc_xcorr_last_error()) > 0);
  }
  std::vector<double> one(3, 1.0);
  CHECK(uc_xcorr_peak(nullptr, 1, &out) == -EINVAL && uc_xcorr_peak(one.data(), 1, nullptr) == -EINVAL);
  CHECK(uc_xcorr_peak(one.data(), 0, &out) == -EINVAL && uc_xcorr_peak(one.data(), UC_XCORR_MAX_LAG + 1, &out) == -EINVAL);
  CHECK(uc_xcorr_abi_version() == UC_XCORR_ABI_VERSION);
  CHECK(uc_xcorr_create(0, nullptr) == -EINVAL);
  uc_xcorr_pair pair = {0, 1};
  double corr[3];
  CHECK(uc_xcorr_correlate(nullptr, corr, UC_XCORR_DTYPE_F32, 2, 8, 0, &pair, 1, 0, 8, 1, corr, 0, nullptr) == -EINVAL);
  uc_xcorr_destroy(nullptr);
  uc_xcorr* xc = nullptr;
  const int rc = uc_xcorr_create(0, &xc);
  if (rc == 0) {
    uc_xcorr_destroy(xc);
    printf("san_xcorr: %d rows; a GPU is visible, uc_xcorr_create succeeded\n", rows);
  } else {
    CHECK(rc == -ENODEV && xc == nullptr && strstr(uc_xcorr_last_error(), "no CPU path"));
    printf("san_xcorr: %d rows; uc_xcorr_create: %d (%s)\n", rows, rc, uc_xcorr_last_error());
  }
  return 0;
}
