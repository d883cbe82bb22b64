// san_retime.cpp -- a stand-alone driver of the host translation unit of libuchirp_retime.so (csrc/uc_retime_api.cpp), built
// with AddressSanitizer and UndefinedBehaviorSanitizer by `make -C ultrasonic-communication_amd sanitize-retime`: the
// fixed-point step over random values, the limits and what lies just beyond them; the table into a buffer of exactly its
// size; every refused argument of uc_retime_rows that is decided before the object is touched; and -- where a GPU is
// missing, as in the sanitizer's container -- the refusal of uc_retime_create.  CPU only: it never launches a kernel.
// With UC_SAN_TEXTS set it prints the library's last error text behind every check, so that two builds can be compared.
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "uchirp_retime.h"

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      printf("san_retime: %s failed (line %d)\n", #c, __LINE__);      \
      return 1;                                                       \
    }                                                                 \
    if (getenv("UC_SAN_TEXTS")) printf("line %d: %s\n", __LINE__, uc_retime_last_error()); \
  } while (0)

// a handle that is not NULL: every refusal below is decided from the arguments alone, before the object is read
static uc_retime* fake() {
  static long long storage[64];
  return reinterpret_cast<uc_retime*>(storage);
}

int main() {
  std::mt19937_64 rng(12);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  const double two30 = 1073741824.0, slope_max = 1.0 / 512.0, inf = std::numeric_limits<double>::infinity();
  int64_t lead = 0, drift = 0;
  int draws = 0;
  for (int i = 0; i < 20000; ++i, ++draws) {
    const double d = u(rng) * std::pow(10.0, 9.0 * u(rng)), s = u(rng) * slope_max * std::pow(10.0, -6.0 * std::fabs(u(rng)));
    if (std::fabs(d) > two30) continue;
    CHECK(uc_retime_fixed(d, s, &lead, &drift) == 0);
    CHECK(std::fabs((double)lead - d * 4294967296.0) <= 0.5 && std::fabs((double)drift - s * 4294967296.0) <= 0.5);
    CHECK(lead >= -(1ll << 62) && lead <= (1ll << 62) && drift >= -(1ll << 23) && drift <= (1ll << 23));
  }
  CHECK(uc_retime_fixed(two30, slope_max, &lead, &drift) == 0 && lead == (1ll << 62) && drift == (1ll << 23));
  CHECK(uc_retime_fixed(-two30, -slope_max, &lead, &drift) == 0 && lead == -(1ll << 62) && drift == -(1ll << 23));
  CHECK(uc_retime_fixed(0.5 / 4294967296.0, 1.5 / 4294967296.0, &lead, &drift) == 0 && lead == 0 && drift == 2);   // ties to even
  CHECK(uc_retime_fixed(5e-324, -5e-324, &lead, &drift) == 0 && lead == 0 && drift == 0);
  lead = drift = 7;
  const double beyond[][2] = {{std::nextafter(two30, inf), 0.0}, {-std::nextafter(two30, inf), 0.0}, {0.0, std::nextafter(slope_max, 1.0)},
                              {0.0, -std::nextafter(slope_max, 1.0)}, {NAN, 0.0}, {inf, 0.0}, {-inf, 0.0}, {0.0, NAN}, {0.0, inf}, {1e300, 1e300}};
  for (const auto& b : beyond) {
    CHECK(uc_retime_fixed(b[0], b[1], &lead, &drift) == -EINVAL && strlen(uc_retime_last_error()) > 0);
    CHECK(lead == 7 && drift == 7);
  }
  CHECK(uc_retime_fixed(1.0, 0.0, nullptr, &drift) == -EINVAL && uc_retime_fixed(1.0, 0.0, &lead, nullptr) == -EINVAL);

  std::vector<float> table(UC_RETIME_TABLE_ROWS * UC_RETIME_COEFS);   // exactly the table: a write past it is a report
  CHECK(uc_retime_table(table.data()) == 0);
  for (int q = 0; q < UC_RETIME_TABLE_ROWS; ++q) {
    double sum = 0.0;
    for (int t = 0; t < UC_RETIME_COEFS; ++t) {
      CHECK(std::isfinite(table[16 * q + t]) && std::fabs(table[16 * q + t]) <= 1.0f);
      sum += table[16 * q + t];
    }
    CHECK(std::fabs(sum - 1.0) < 1e-3);
  }
  CHECK(table[7] == 1.0f && table[16 * 256 + 8] == 1.0f && table[8] == 0.0f && table[16 * 256 + 7] == 0.0f);
  CHECK(uc_retime_table(nullptr) == -EINVAL);

  // uc_retime_rows: what is refused from the arguments alone.  `dev` is host memory: a call that passed every check before
  // the test for device memory is refused there (or, without a HIP runtime, at hipSetDevice), never run.
  std::vector<float> dev(64);
  uc_retime_line ok = {2.25, 40e-6, 0, 0};
  std::vector<uc_retime_line> lines(2, ok);   // exactly two lines: a read past them is a report
  const size_t big = (size_t)1 << 41;
  struct Case {
    const char* name;
    uc_retime* h;
    const void* in;
    int dtype;
    size_t n_mics, n_in, in_stride;
    const uc_retime_line* ln;
    size_t n_lines;
    float* out;
    uint64_t out_first;
    size_t n_out, out_stride;
    uint64_t in_first;
  };
  float* const o = dev.data() + 32;
  const Case cases[] = {
      {"retime NULL", nullptr, dev.data(), 1, 1, 16, 0, lines.data(), 2, o, 0, 16, 0, 0},
      {"in NULL", fake(), nullptr, 1, 1, 16, 0, lines.data(), 2, o, 0, 16, 0, 0},
      {"out NULL", fake(), dev.data(), 1, 1, 16, 0, lines.data(), 2, nullptr, 0, 16, 0, 0},
      {"lines NULL", fake(), dev.data(), 1, 1, 16, 0, nullptr, 2, o, 0, 16, 0, 0},
      {"dtype 2", fake(), dev.data(), 2, 1, 16, 0, lines.data(), 2, o, 0, 16, 0, 0},
      {"dtype -1", fake(), dev.data(), -1, 1, 16, 0, lines.data(), 2, o, 0, 16, 0, 0},
      {"no microphones", fake(), dev.data(), 1, 0, 16, 0, lines.data(), 2, o, 0, 16, 0, 0},
      {"too many microphones", fake(), dev.data(), 1, (size_t)1 << 32, 16, 0, lines.data(), 2, o, 0, 16, 0, 0},
      {"no lines", fake(), dev.data(), 1, 1, 16, 0, lines.data(), 0, o, 0, 16, 0, 0},
      {"too many lines", fake(), dev.data(), 1, 1, 16, 0, lines.data(), (size_t)1 << 32, o, 0, 16, 0, 0},
      {"no input samples", fake(), dev.data(), 1, 1, 0, 0, lines.data(), 2, o, 0, 16, 0, 0},
      {"no output samples", fake(), dev.data(), 1, 1, 16, 0, lines.data(), 2, o, 0, 0, 0, 0},
      {"n_in too large", fake(), dev.data(), 1, 1, big, 0, lines.data(), 2, o, 0, 16, 0, 0},
      {"in_first too large", fake(), dev.data(), 1, 1, 16, 0, lines.data(), 2, o, 0, 16, 0, (1ull << 52) + 1},
      {"out_first + n_out > 2^38", fake(), dev.data(), 1, 1, 16, 0, lines.data(), 2, o, (1ull << 38) - 15, 16, 0, 0},
      {"out_first > 2^38", fake(), dev.data(), 1, 1, 16, 0, lines.data(), 2, o, (1ull << 38) + 1, 16, 0, 0},
      {"out_first + n_out wraps", fake(), dev.data(), 1, 1, 16, 0, lines.data(), 2, o, ~0ull - 3, 16, 0, 0},
      {"n_out > 2^38", fake(), dev.data(), 1, 1, 16, 0, lines.data(), 2, o, 0, ((size_t)1 << 38) + 1, 0, 0},
      {"in_stride < n_in", fake(), dev.data(), 1, 1, 16, 15, lines.data(), 2, o, 0, 16, 0, 0},
      {"out_stride < n_out", fake(), dev.data(), 1, 1, 16, 0, lines.data(), 2, o, 0, 16, 15, 0},
      {"in_stride too large", fake(), dev.data(), 1, 1, 16, big, lines.data(), 2, o, 0, 16, 0, 0},
      {"out_stride too large", fake(), dev.data(), 1, 1, 16, 0, lines.data(), 2, o, 0, 16, big, 0},
      {"out overlaps in", fake(), dev.data(), 1, 1, 16, 0, lines.data(), 2, dev.data() + 8, 0, 16, 0, 0},
  };
  int refused = 0;
  for (const Case& c : cases) {
    const int rc = uc_retime_rows(c.h, c.in, c.dtype, c.n_mics, c.in_first, c.n_in, c.in_stride, c.ln, c.n_lines, c.out, c.out_first,
                                  c.n_out, c.out_stride, nullptr);
    if (getenv("UC_SAN_TEXTS")) printf("%s: %d: %s\n", c.name, rc, uc_retime_last_error());   // to compare the texts of two builds
    if (rc != -EINVAL || strlen(uc_retime_last_error()) == 0) {
      printf("san_retime: %s: rc %d (%s)\n", c.name, rc, uc_retime_last_error());
      return 1;
    }
    ++refused;
  }
  // one bad line at a time, the second of two
  const uc_retime_line bad[] = {{2.25, 40e-6, 1, 0},   // mic >= n_mics
                                {2.25, 40e-6, 0, 1},   // reserved != 0
                                {NAN, 0.0, 0, 0},         {inf, 0.0, 0, 0},          {0.0, NAN, 0, 0},
                                {0.0, -inf, 0, 0},        {two30 + 1.0, 0.0, 0, 0},  {-two30 - 1.0, 0.0, 0, 0},
                                {0.0, std::nextafter(slope_max, 1.0), 0, 0},         {0.0, -std::nextafter(slope_max, 1.0), 0, 0}};
  for (const uc_retime_line& b : bad) {
    lines[1] = b;
    CHECK(uc_retime_rows(fake(), dev.data(), 1, 1, 0, 16, 0, lines.data(), 2, o, 0, 16, 0, nullptr) == -EINVAL);
    CHECK(strstr(uc_retime_last_error(), "line 1"));
    ++refused;
  }
  lines[1] = ok;

  CHECK(uc_retime_abi_version() == UC_RETIME_ABI_VERSION);
  CHECK(uc_retime_create(0, nullptr) == -EINVAL);
  uc_retime_destroy(nullptr);
  uc_retime* rt = nullptr;
  const int rc = uc_retime_create(0, &rt);
  if (rc == 0) {
    // with a GPU the checks that need the object run too: host memory is no device memory
    CHECK(uc_retime_rows(rt, dev.data(), 1, 1, 0, 16, 0, lines.data(), 2, o, 0, 16, 0, nullptr) == -EINVAL);
    uc_retime_destroy(rt);
    printf("san_retime: %d draws, %d refusals; a GPU is visible, uc_retime_create succeeded\n", draws, refused);
  } else {
    CHECK(rc == -ENODEV && rt == nullptr && strstr(uc_retime_last_error(), "no CPU path"));
    printf("san_retime: %d draws, %d refusals; uc_retime_create: %d (%s)\n", draws, refused, rc, uc_retime_last_error());
  }
  return 0;
}
