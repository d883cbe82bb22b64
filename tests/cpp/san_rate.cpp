// san_rate.cpp -- a stand-alone driver of the host translation unit of libuchirp_rate.so (csrc/uc_rate_api.cpp), built with
// AddressSanitizer and UndefinedBehaviorSanitizer by `make -C ultrasonic-communication_amd sanitize-rate`: the plan of the
// three sound-card rates, of random ratios and of what lies just beyond the limits; the table into a buffer of exactly its
// size; the step and the span against 128-bit arithmetic up to the last sample number; every refused argument of
// uc_rate_convert that is decided before the object is touched; and -- where a GPU is missing, as in the sanitizer's
// container -- the refusal of uc_rate_create.  CPU only: it never launches a kernel.
// With UC_SAN_TEXTS set it prints the library's last error text behind every check, so that two builds can be compared.
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <vector>

#include "uchirp_rate.h"

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      printf("san_rate: %s failed (line %d)\n", #c, __LINE__);        \
      return 1;                                                       \
    }                                                                 \
    if (getenv("UC_SAN_TEXTS")) printf("line %d: %s\n", __LINE__, uc_rate_last_error()); \
  } while (0)

// a handle that is not NULL: every refusal below is decided from the arguments alone, before the object is read
static uc_rate* fake() {
  static long long storage[64];
  return reinterpret_cast<uc_rate*>(storage);
}

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  uc_rate_info f;
  // ---- the plan
  CHECK(uc_rate_plan(78125, 44100, 24, 9.0, &f) == 0 && f.up == 3125 && f.down == 1764 && f.taps == 49 && f.centre == 75000 && f.table_len == 153125);
  CHECK(uc_rate_plan(78125, 48000, 24, 9.0, &f) == 0 && f.up == 625 && f.down == 384 && f.taps == 49);
  CHECK(uc_rate_plan(78125, 96000, 24, 9.0, &f) == 0 && f.up == 625 && f.down == 768 && f.taps == 59 && f.centre == 24 * 768);
  std::mt19937_64 rng(16);
  int plans = 0, refused = 0;
  for (int i = 0; i < 20000; ++i) {
    const uint32_t up = 1 + (uint32_t)(rng() % 5000), down = 1 + (uint32_t)(rng() % 5000), half = (uint32_t)(rng() % 40);
    const uint32_t g = std::gcd(up, down), u = up / g, d = down / g, q = u > d ? u : d;
    const bool ok = u != d && q <= 4096 && half >= 4 && half <= 32 && 2 * half * q / u + 1 <= 128;
    uc_rate_info r = {7, 7, 7, 7, 7, 7};
    const int rc = uc_rate_plan(up, down, half, 9.0, &r);
    CHECK(rc == (ok ? 0 : -EINVAL));
    if (ok) {
      CHECK(r.up == u && r.down == d && r.half == half && r.taps == 2 * half * q / u + 1 && r.centre == half * q && r.table_len == u * r.taps);
      CHECK(r.table_len <= UC_RATE_TABLE_MAX);
      ++plans;
    } else {
      CHECK(r.up == 7 && r.table_len == 7 && strlen(uc_rate_last_error()) > 0);
      ++refused;
    }
  }
  const struct { uint32_t up, down, half; double beta; } beyond[] = {
      {0, 5, 24, 9.0}, {5, 0, 24, 9.0}, {5, 5, 24, 9.0}, {78125, 78125, 24, 9.0}, {4097, 4096, 24, 9.0}, {4096, 4097, 4, 9.0}, {3, 2, 3, 9.0},
      {3, 2, 33, 9.0}, {3, 2, 24, NAN}, {3, 2, 24, inf}, {3, 2, 24, -inf}, {3, 2, 24, -1e-300}, {3, 2, 24, std::nextafter(100.0, inf)},
      {1, 16, 4, 9.0}, {1, 3, 32, 9.0}, {0xFFFFFFFFu, 0xFFFFFFFEu, 24, 9.0}};
  for (const auto& b : beyond) {
    uc_rate_info r = {7, 7, 7, 7, 7, 7};
    CHECK(uc_rate_plan(b.up, b.down, b.half, b.beta, &r) == -EINVAL && strlen(uc_rate_last_error()) > 0 && r.up == 7 && r.taps == 7);
    ++refused;
  }
  CHECK(uc_rate_plan(3, 2, 24, 9.0, nullptr) == -EINVAL);
  CHECK(uc_rate_plan(4096, 4095, 32, 100.0, &f) == 0 && uc_rate_plan(4095, 4096, 32, 0.0, &f) == 0 && uc_rate_plan(1, 15, 4, 9.0, &f) == 0 && f.taps == 121);

  // ---- the table: into a buffer of exactly its size (a write past it is a report); unity gain per phase; the largest ones
  const struct { uint32_t up, down, half; double beta; } tables[] = {{78125, 44100, 24, 9.0}, {78125, 96000, 24, 9.0}, {5, 13, 24, 9.0}, {7, 5, 4, 0.0},
                                                                     {4096, 4095, 32, 100.0}, {4095, 4096, 32, 14.0}, {1, 15, 4, 5.0}};
  for (const auto& t : tables) {
    CHECK(uc_rate_plan(t.up, t.down, t.half, t.beta, &f) == 0);
    std::vector<float> tab(f.table_len);
    CHECK(uc_rate_table(&f, t.beta, tab.data(), tab.size()) == 0);
    double total = 0.0;
    for (float v : tab) {
      CHECK(std::isfinite(v) && std::fabs(v) <= 1.5f);
      total += v;
    }
    CHECK(std::fabs(total - (double)f.up) < 1e-3 * f.up);                 // sum h = up
    const uint32_t q = f.up > f.down ? f.up : f.down, n_h = 2 * f.half * q + 1;
    for (uint32_t p = 0; p < f.up; ++p)
      for (uint32_t j = 0; j < f.taps; ++j)
        if (p + j * f.up >= n_h) CHECK(tab[(size_t)p * f.taps + j] == 0.0f);
    CHECK(uc_rate_table(&f, t.beta, tab.data(), tab.size() - 1) == -EINVAL && uc_rate_table(&f, t.beta, tab.data(), tab.size() + 1) == -EINVAL);
    CHECK(uc_rate_table(&f, NAN, tab.data(), tab.size()) == -EINVAL && uc_rate_table(&f, t.beta, nullptr, tab.size()) == -EINVAL);
    CHECK(uc_rate_table(nullptr, t.beta, tab.data(), tab.size()) == -EINVAL);
  }

  // ---- the step, the span, the count
  const uint64_t end = 1ull << 38;
  int steps = 0;
  for (const auto& t : tables) {
    CHECK(uc_rate_plan(t.up, t.down, t.half, t.beta, &f) == 0);
    for (int i = 0; i < 4000; ++i) {
      const uint64_t m = i < 1000 ? (uint64_t)i : i < 2000 ? end - 1 - (uint64_t)(i - 1000) : rng() % end;
      int64_t k = -1;
      uint32_t p = 7;
      CHECK(uc_rate_step(&f, m, &k, &p) == 0);
      const unsigned __int128 pos = (unsigned __int128)m * f.down + f.centre;
      CHECK((unsigned __int128)k * f.up + p == pos && p < f.up && k >= 0);
      const size_t n = 1 + (size_t)(rng() % 4096);
      if (m + n <= end) {
        int64_t lo = 0, hi = 0, k2 = 0;
        CHECK(uc_rate_span(&f, m, n, &lo, &hi) == 0 && lo == k - (int64_t)f.taps + 1);
        CHECK(uc_rate_step(&f, m + n - 1, &k2, &p) == 0 && hi == k2 + 1 && hi > lo);
      }
      ++steps;
    }
    int64_t k = 7, lo = 7, hi = 7;
    uint32_t p = 7;
    CHECK(uc_rate_step(&f, end, &k, &p) == -EINVAL && uc_rate_step(&f, ~0ull, &k, &p) == -EINVAL && k == 7 && p == 7);
    CHECK(uc_rate_step(nullptr, 0, &k, &p) == -EINVAL && uc_rate_step(&f, 0, nullptr, &p) == -EINVAL && uc_rate_step(&f, 0, &k, nullptr) == -EINVAL);
    CHECK(uc_rate_span(&f, 0, 0, &lo, &hi) == -EINVAL && uc_rate_span(&f, end - 4, 5, &lo, &hi) == -EINVAL && uc_rate_span(&f, ~0ull - 1, 5, &lo, &hi) == -EINVAL);
    CHECK(uc_rate_span(&f, 0, (size_t)end + 1, &lo, &hi) == -EINVAL && uc_rate_span(nullptr, 0, 5, &lo, &hi) == -EINVAL);
    CHECK(uc_rate_span(&f, 0, 5, nullptr, &hi) == -EINVAL && uc_rate_span(&f, 0, 5, &lo, nullptr) == -EINVAL && lo == 7 && hi == 7);
    CHECK(uc_rate_span(&f, end - 5, 5, &lo, &hi) == 0 && uc_rate_span(&f, 0, (size_t)end, &lo, &hi) == 0 && lo == (int64_t)(f.centre / f.up) - (int64_t)f.taps + 1);
    const uint64_t counts[] = {0, 1, 2, 1500, f.down, (uint64_t)f.down + 1, 88200, 1ull << 40};
    for (uint64_t n : counts)
      CHECK(uc_rate_count(&f, n) == (int64_t)(((unsigned __int128)n * f.up + f.down - 1) / f.down));
    CHECK(uc_rate_count(&f, (1ull << 40) + 1) == -EINVAL && uc_rate_count(nullptr, 5) == -EINVAL);
    uc_rate_info bad = f;
    bad.taps += 1;
    CHECK(uc_rate_step(&bad, 0, &k, &p) == -EINVAL && uc_rate_span(&bad, 0, 5, &lo, &hi) == -EINVAL && uc_rate_count(&bad, 5) == -EINVAL);
    bad = f;
    bad.up *= 2;
    bad.down *= 2;
    CHECK(uc_rate_step(&bad, 0, &k, &p) == -EINVAL);
    memset(&bad, 0, sizeof(bad));
    CHECK(uc_rate_step(&bad, 0, &k, &p) == -EINVAL && uc_rate_count(&bad, 5) == -EINVAL);
  }

  // ---- uc_rate_convert: what is refused from the arguments alone.  `dev` is host memory: a call that passed every check
  // before the test for device memory is refused there (or, without a HIP runtime, at hipSetDevice), never run.
  std::vector<float> dev(64);
  const size_t big = (size_t)1 << 41;
  struct Case {
    const char* name;
    uc_rate* h;
    const void* in;
    int dtype;
    size_t n_rows, n_in, in_stride;
    float* out;
    uint64_t out_first;
    size_t n_out, out_stride;
    uint64_t in_first;
  };
  float* const o = dev.data() + 32;
  const Case cases[] = {
      {"rate NULL", nullptr, dev.data(), 1, 1, 16, 0, o, 0, 16, 0, 0},
      {"in NULL", fake(), nullptr, 1, 1, 16, 0, o, 0, 16, 0, 0},
      {"out NULL", fake(), dev.data(), 1, 1, 16, 0, nullptr, 0, 16, 0, 0},
      {"dtype 2", fake(), dev.data(), 2, 1, 16, 0, o, 0, 16, 0, 0},
      {"dtype -1", fake(), dev.data(), -1, 1, 16, 0, o, 0, 16, 0, 0},
      {"no rows", fake(), dev.data(), 1, 0, 16, 0, o, 0, 16, 0, 0},
      {"too many rows", fake(), dev.data(), 1, (size_t)1 << 32, 16, 0, o, 0, 16, 0, 0},
      {"no input samples", fake(), dev.data(), 1, 1, 0, 0, o, 0, 16, 0, 0},
      {"no output samples", fake(), dev.data(), 1, 1, 16, 0, o, 0, 0, 0, 0},
      {"n_in too large", fake(), dev.data(), 1, 1, big, 0, o, 0, 16, 0, 0},
      {"in_first too large", fake(), dev.data(), 1, 1, 16, 0, o, 0, 16, 0, (1ull << 52) + 1},
      {"out_first + n_out > 2^38", fake(), dev.data(), 1, 1, 16, 0, o, (1ull << 38) - 15, 16, 0, 0},
      {"out_first > 2^38", fake(), dev.data(), 1, 1, 16, 0, o, (1ull << 38) + 1, 16, 0, 0},
      {"out_first + n_out wraps", fake(), dev.data(), 1, 1, 16, 0, o, ~0ull - 3, 16, 0, 0},
      {"n_out > 2^38", fake(), dev.data(), 1, 1, 16, 0, o, 0, ((size_t)1 << 38) + 1, 0, 0},
      {"in_stride < n_in", fake(), dev.data(), 1, 1, 16, 15, o, 0, 16, 0, 0},
      {"out_stride < n_out", fake(), dev.data(), 1, 1, 16, 0, o, 0, 16, 15, 0},
      {"in_stride too large", fake(), dev.data(), 1, 1, 16, big, o, 0, 16, 0, 0},
      {"out_stride too large", fake(), dev.data(), 1, 1, 16, 0, o, 0, 16, big, 0},
      {"out overlaps in", fake(), dev.data(), 1, 1, 16, 0, dev.data() + 8, 0, 16, 0, 0},
      {"out overlaps in (PCM)", fake(), dev.data(), 0, 1, 16, 0, dev.data() + 7, 0, 16, 0, 0},
  };
  for (const Case& c : cases) {
    const int rc = uc_rate_convert(c.h, c.in, c.dtype, c.n_rows, c.in_first, c.n_in, c.in_stride, c.out, c.out_first, c.n_out, c.out_stride, nullptr);
    if (getenv("UC_SAN_TEXTS")) printf("%s: %d: %s\n", c.name, rc, uc_rate_last_error());   // to compare the texts of two builds
    if (rc != -EINVAL || strlen(uc_rate_last_error()) == 0) {
      printf("san_rate: %s: rc %d (%s)\n", c.name, rc, uc_rate_last_error());
      return 1;
    }
    ++refused;
  }

  CHECK(uc_rate_abi_version() == UC_RATE_ABI_VERSION);
  uc_rate* cv = fake();
  CHECK(uc_rate_create(0, 3, 2, 24, 9.0, nullptr) == -EINVAL);
  CHECK(uc_rate_create(0, 5, 5, 24, 9.0, &cv) == -EINVAL && cv == nullptr);      // a refused ratio is refused with or without a GPU
  cv = fake();
  CHECK(uc_rate_create(0, 3, 2, 3, 9.0, &cv) == -EINVAL && cv == nullptr);
  uc_rate_destroy(nullptr);
  const int rc = uc_rate_create(0, 78125, 44100, 24, 9.0, &cv);
  if (rc == 0) {
    // with a GPU the checks that need the object run too: host memory is no device memory
    CHECK(uc_rate_convert(cv, dev.data(), 1, 1, 0, 16, 0, o, 0, 16, 0, nullptr) == -EINVAL);
    uc_rate_destroy(cv);
    printf("san_rate: %d plans, %d steps, %d refusals; a GPU is visible, uc_rate_create succeeded\n", plans, steps, refused);
  } else {
    CHECK(rc == -ENODEV && cv == nullptr && strstr(uc_rate_last_error(), "no CPU path"));
    printf("san_rate: %d plans, %d steps, %d refusals; uc_rate_create: %d (%s)\n", plans, steps, refused, rc, uc_rate_last_error());
  }
  return 0;
}
