// san_wcorr.cpp -- a stand-alone driver of the host translation unit of libuchirp_wcorr.so (csrc/uc_wcorr_api.cpp), built
// with AddressSanitizer and UndefinedBehaviorSanitizer by `make -C ultrasonic-communication_amd sanitize-wcorr`: the band
// weights into a buffer of exactly their size (the formula, a brick wall, the tail shares and what is refused);
// uc_wcorr_peak on rows of exactly their size; every refused argument of uc_wcorr_windows that is decided before the
// object is touched; and -- where a GPU is missing, as in the sanitizer's container -- the refusal of uc_wcorr_create.
// CPU only: it never launches a kernel.  With UC_SAN_TEXTS set it prints the library's last error text behind every
// check, so that two builds can be compared.
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "uchirp_wcorr.h"

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      printf("san_wcorr: %s failed (line %d)\n", #c, __LINE__);      \
      return 1;                                                      \
    }                                                                \
    if (getenv("UC_SAN_TEXTS")) printf("line %d: %s\n", __LINE__, uc_wcorr_last_error()); \
  } while (0)

// a handle that is not NULL: every refusal below is decided from the arguments alone, before the object is used
static uc_wcorr* fake() {
  static long long storage[128];
  return reinterpret_cast<uc_wcorr*>(storage);
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  int tables = 0, peaks = 0;
  {  // the band of the chirps: 1 inside, cos^2 edges, 0 beyond; the tail falls with the guard and is 0 from 1024 on
    std::vector<float> w(UC_WCORR_BINS);   // exactly the table: a write past it is a report
    double tail = -1.0, last = 2.0;
    const uint32_t guards[] = {0, 32, 64, 128, 256, 1023, 1024, 5000, 0xFFFFFFFFu};
    for (uint32_t g : guards) {
      CHECK(uc_wcorr_band_weights(78125.0, 16000.0, 19000.0, 1000.0, g, w.data(), &tail) == 0);
      CHECK(tail >= 0.0 && tail <= last && (g < 1024 || tail == 0.0));
      last = tail;
      ++tables;
    }
    const double fk = 78125.0 / 2048.0;
    for (int k = 0; k < UC_WCORR_BINS; ++k) {
      const double f = k * fk, d = f < 16000.0 ? 16000.0 - f : f > 19000.0 ? f - 19000.0 : 0.0;
      const double c = std::cos(0.5 * 3.14159265358979323846 * d / 1000.0);
      const double want = d == 0.0 ? 1.0 : d < 1000.0 ? c * c : 0.0;
      CHECK(std::fabs((double)w[k] - want) <= 1e-7);
    }
    CHECK(uc_wcorr_band_weights(78125.0, 16000.0, 19000.0, 1000.0, 128, w.data(), nullptr) == 0);   // no tail asked
    CHECK(uc_wcorr_band_weights(78125.0, 16000.0, 19000.0, 0.0, 128, w.data(), &tail) == 0);        // a brick wall
    for (int k = 0; k < UC_WCORR_BINS; ++k) CHECK(w[k] == (k * fk >= 16000.0 && k * fk <= 19000.0 ? 1.0f : 0.0f));
    CHECK(uc_wcorr_band_weights(78125.0, 17000.5, 17000.5, 0.0, 0, w.data(), &tail) == 0 && tail == 0.0);   // no bin: zeros
    CHECK(uc_wcorr_band_weights(78125.0, 0.0, 1e9, 0.0, 0, w.data(), &tail) == 0 && tail < 1e-20 && w[0] == 1.0f && w[1024] == 1.0f);   // ones: an impulse
    tables += 4;
    CHECK(uc_wcorr_band_weights(78125.0, 19000.0, 16000.0, 1000.0, 0, w.data(), &tail) == -EINVAL && strlen(uc_wcorr_last_error()) > 0);
    CHECK(uc_wcorr_band_weights(78125.0, 16000.0, 19000.0, -1.0, 0, w.data(), &tail) == -EINVAL);
    CHECK(uc_wcorr_band_weights(78125.0, -1.0, 19000.0, 0.0, 0, w.data(), &tail) == -EINVAL);
    CHECK(uc_wcorr_band_weights(0.0, 16000.0, 19000.0, 0.0, 0, w.data(), &tail) == -EINVAL);
    CHECK(uc_wcorr_band_weights(-78125.0, 16000.0, 19000.0, 0.0, 0, w.data(), &tail) == -EINVAL);
    CHECK(uc_wcorr_band_weights(nan, 16000.0, 19000.0, 0.0, 0, w.data(), &tail) == -EINVAL);
    CHECK(uc_wcorr_band_weights(78125.0, nan, 19000.0, 0.0, 0, w.data(), &tail) == -EINVAL);
    CHECK(uc_wcorr_band_weights(78125.0, 16000.0, nan, 0.0, 0, w.data(), &tail) == -EINVAL);
    CHECK(uc_wcorr_band_weights(78125.0, 16000.0, 19000.0, nan, 0, w.data(), &tail) == -EINVAL);
    CHECK(uc_wcorr_band_weights(78125.0, 16000.0, inf, 0.0, 0, w.data(), &tail) == -EINVAL);
    CHECK(uc_wcorr_band_weights(78125.0, 16000.0, 19000.0, 0.0, 0, nullptr, &tail) == -EINVAL);
  }
  {  // the peak rule on rows of exactly their size
    std::unique_ptr<uc_wcorr_peak_t> out(new uc_wcorr_peak_t);
    std::vector<double> r = {1.0, 2.0, 3.0, 2.0, 1.0};
    CHECK(uc_wcorr_peak(r.data(), 2, out.get()) == 0);
    CHECK(out->flags == 0 && out->lag == 0 && out->delay_samples == 0.0 && out->height == 3.0 && out->runner_up == 0.0);
    std::vector<double> fall = {3.0, 2.0, 1.0};
    CHECK(uc_wcorr_peak(fall.data(), 1, out.get()) == 0 && out->flags == (UC_WCORR_NO_PEAK | UC_WCORR_AT_EDGE) && out->height == 0.0);
    std::vector<double> wide(2 * UC_WCORR_MAX_LAG + 1);
    for (size_t k = 0; k < wide.size(); ++k) wide[k] = std::cos(2.0 * 3.14159265358979323846 * ((double)k - 500.3) / 4.46) * std::exp(-0.5 * std::pow(((double)k - 500.3) / 9.0, 2.0));
    CHECK(uc_wcorr_peak(wide.data(), UC_WCORR_MAX_LAG, out.get()) == 0);
    CHECK(out->flags == 0 && out->lag == 500 - 512 && std::fabs(out->delay_samples - (500.3 - 512.0)) < 0.05 && out->runner_up > 0.5 && out->runner_up < 1.0);
    r[3] = nan;
    CHECK(uc_wcorr_peak(r.data(), 2, out.get()) == -EINVAL && strlen(uc_wcorr_last_error()) > 0);
    r[3] = inf;
    CHECK(uc_wcorr_peak(r.data(), 2, out.get()) == -EINVAL);
    r[3] = 2.0;
    CHECK(uc_wcorr_peak(nullptr, 2, out.get()) == -EINVAL && uc_wcorr_peak(r.data(), 2, nullptr) == -EINVAL);
    CHECK(uc_wcorr_peak(r.data(), 0, out.get()) == -EINVAL && uc_wcorr_peak(wide.data(), 513, out.get()) == -EINVAL);
    peaks = 9;
  }

  // uc_wcorr_windows: what is refused from the arguments alone.  `dev` is host memory: a call that passed every check before
  // the test for device memory is refused there (or, without a HIP runtime, at hipSetDevice), never run.
  std::vector<float> dev(4096);
  std::vector<uc_wcorr_pair> pairs(2, uc_wcorr_pair{0, 1});   // exactly two pairs: a read past them is a report
  std::vector<double> corr_mem(2 * 3 * 17);
  double* const co = corr_mem.data();
  std::vector<float> ones(UC_WCORR_BINS, 1.0f), bad_nan(ones), bad_inf(ones), bad_last(ones);   // exactly the table
  bad_nan[0] = std::numeric_limits<float>::quiet_NaN();
  bad_inf[700] = std::numeric_limits<float>::infinity();
  bad_last[UC_WCORR_BINS - 1] = -std::numeric_limits<float>::infinity();
  const size_t big = (size_t)1 << 41;
  struct Case {
    const char* name;
    uc_wcorr* h;
    const void* in;
    int dtype;
    size_t n_mics, n_in, in_stride;
    const uc_wcorr_pair* pr;
    size_t n_pairs, first, window_len, hop, n_windows;
    uint32_t L, guard;
    const float* w;
    double* corr;
    size_t corr_stride;
  };
  const void* in = dev.data();
  const float* w1 = ones.data();
  const Case cases[] = {
      {"wcorr NULL", nullptr, in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, 2, w1, co, 0},
      {"in NULL", fake(), nullptr, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, 2, w1, co, 0},
      {"corr NULL", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, 2, w1, nullptr, 0},
      {"pairs NULL", fake(), in, 1, 2, 64, 0, nullptr, 2, 0, 16, 16, 3, 4, 2, w1, co, 0},
      {"dtype 2", fake(), in, 2, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, 2, w1, co, 0},
      {"dtype -1", fake(), in, -1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, 2, w1, co, 0},
      {"no microphones", fake(), in, 1, 0, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, 2, w1, co, 0},
      {"too many microphones", fake(), in, 1, (size_t)1 << 32, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, 2, w1, co, 0},
      {"no pairs", fake(), in, 1, 2, 64, 0, pairs.data(), 0, 0, 16, 16, 3, 4, 2, w1, co, 0},
      {"too many pairs", fake(), in, 1, 2, 64, 0, pairs.data(), (size_t)1 << 32, 0, 16, 16, 3, 4, 2, w1, co, 0},
      {"no windows", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 0, 4, 2, w1, co, 0},
      {"too many windows", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, (size_t)1 << 32, 4, 2, w1, co, 0},
      {"pairs * windows too many", fake(), in, 1, 2, big / 2, 0, pairs.data(), 2, 0, 1, 1, (size_t)1 << 31, 4, 2, w1, co, 0},
      {"no input samples", fake(), in, 1, 2, 0, 0, pairs.data(), 2, 0, 16, 16, 3, 4, 2, w1, co, 0},
      {"window_len 0", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 0, 16, 3, 4, 2, w1, co, 0},
      {"hop 0", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 0, 3, 4, 2, w1, co, 0},
      {"n_in too large", fake(), in, 1, 2, big, 0, pairs.data(), 2, 0, 16, 16, 3, 4, 2, w1, co, 0},
      {"first > n_in", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 65, 16, 16, 1, 4, 2, w1, co, 0},
      {"first + window_len > n_in", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 49, 16, 16, 1, 4, 2, w1, co, 0},
      {"the last window past n_in", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 17, 16, 16, 3, 4, 2, w1, co, 0},
      {"the last window past n_in, gaps", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 25, 3, 4, 2, w1, co, 0},
      {"hop wraps", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, ~(size_t)0, 3, 4, 2, w1, co, 0},
      {"max_lag 0", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 0, 2, w1, co, 0},
      {"max_lag 513", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 513, 0, w1, co, 0},
      {"max_lag + guard 513", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, 509, w1, co, 0},
      {"guard wraps", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, 0xFFFFFFFEu, w1, co, 0},
      {"a weight is NaN", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, 2, bad_nan.data(), co, 0},
      {"a weight is infinite", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, 2, bad_inf.data(), co, 0},
      {"the last weight is infinite", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, 2, bad_last.data(), co, 0},
      {"in_stride < n_in", fake(), in, 1, 2, 64, 63, pairs.data(), 2, 0, 16, 16, 3, 4, 2, w1, co, 0},
      {"corr_stride < lags", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, 2, w1, co, 8},
      {"in_stride too large", fake(), in, 1, 2, 64, big, pairs.data(), 2, 0, 16, 16, 3, 4, 2, w1, co, 0},
      {"corr_stride too large", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, 2, w1, co, big},
      {"corr overlaps in", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, 2, w1, reinterpret_cast<double*>(dev.data() + 32), 0},
  };
  int refused = 0;
  for (const Case& c : cases) {
    const int rc = uc_wcorr_windows(c.h, c.in, c.dtype, c.n_mics, c.n_in, c.in_stride, c.pr, c.n_pairs, c.first, c.window_len, c.hop,
                                    c.n_windows, c.L, c.guard, c.w, c.corr, c.corr_stride, nullptr);
    if (getenv("UC_SAN_TEXTS")) printf("%s: %d: %s\n", c.name, rc, uc_wcorr_last_error());   // to compare the texts of two builds
    if (rc != -EINVAL || strlen(uc_wcorr_last_error()) == 0) {
      printf("san_wcorr: %s: rc %d (%s)\n", c.name, rc, uc_wcorr_last_error());
      return 1;
    }
    ++refused;
  }
  // one bad pair at a time, the second of two
  const uc_wcorr_pair bad[] = {{2, 0}, {0, 2}, {0xFFFFFFFFu, 0}};
  for (const uc_wcorr_pair& b : bad) {
    pairs[1] = b;
    CHECK(uc_wcorr_windows(fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, 2, nullptr, co, 0, nullptr) == -EINVAL);
    CHECK(strstr(uc_wcorr_last_error(), "pair 1"));
    ++refused;
  }
  pairs[1] = uc_wcorr_pair{1, 1};

  CHECK(uc_wcorr_abi_version() == UC_WCORR_ABI_VERSION);
  CHECK(uc_wcorr_create(0, nullptr) == -EINVAL);
  uc_wcorr_destroy(nullptr);
  uc_wcorr* wc = nullptr;
  const int rc = uc_wcorr_create(0, &wc);
  if (rc == 0) {
    // with a GPU the checks that need the object run too: host memory is no device memory
    CHECK(uc_wcorr_windows(wc, in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, 2, w1, co, 0, nullptr) == -EINVAL);
    uc_wcorr_destroy(wc);
    printf("san_wcorr: %d tables, %d peaks, %d refusals; a GPU is visible, uc_wcorr_create succeeded\n", tables, peaks, refused);
  } else {
    CHECK(rc == -ENODEV && wc == nullptr && strstr(uc_wcorr_last_error(), "no CPU path"));
    printf("san_wcorr: %d tables, %d peaks, %d refusals; uc_wcorr_create: %d (%s)\n", tables, peaks, refused, rc, uc_wcorr_last_error());
  }
  return 0;
}
