// san_spec.cpp -- a stand-alone driver of the host translation unit of libuchirp_spec.so (csrc/uc_spec_api.cpp), built with
// AddressSanitizer and UndefinedBehaviorSanitizer by `make -C ultrasonic-communication_amd sanitize-spec`: the frame count
// against 128-bit arithmetic up to the largest rows, the plan of random and of extreme parameter structs, every refused
// argument of uc_spec_run and uc_spec_set_window that is decided before the object is touched; and -- where a GPU is
// missing, as in the sanitizer's container -- the refusal of uc_spec_create.  CPU only: it never launches a kernel.
// With UC_SAN_TEXTS set it prints the library's last error text behind every check, so that two builds can be compared.
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "uchirp_spec.h"

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      printf("san_spec: %s failed (line %d)\n", #c, __LINE__);        \
      return 1;                                                       \
    }                                                                 \
    if (getenv("UC_SAN_TEXTS")) printf("line %d: %s\n", __LINE__, uc_spec_last_error()); \
  } while (0)

// a handle that is not NULL: every refusal below is decided from the arguments alone, before the object is read
static uc_spec* fake() {
  static long long storage[64];
  return reinterpret_cast<uc_spec*>(storage);
}

static uc_spec_params defaults() {
  uc_spec_params p;
  memset(&p, 0, sizeof(p));
  p.frame_len = 2048;
  p.hop = 2048;
  p.n_bins = 1025;
  p.kind = UC_SPEC_MAG;
  p.scale = 1.0f;
  p.floor = 1e-20f;
  p.db_mul = 10.0f;
  return p;
}

int main() {
  const float inf = std::numeric_limits<float>::infinity();
  std::mt19937_64 rng(18);
  int counts = 0, plans = 0, refused = 0;

  // ---- the frame count
  CHECK(uc_spec_frames(2048, 0, 2048, 2048) == 1 && uc_spec_frames(2049, 0, 2048, 2048) == 2 && uc_spec_frames(4096, -2047, 2048, 1) == 6143);
  CHECK(uc_spec_frames(1, 0, 1, 1) == 1 && uc_spec_frames(1ull << 40, -2047, 2048, 1) == (int64_t)(1ull << 40) + 2047);
  CHECK(uc_spec_frames(1ull << 40, 0, 1, 0xFFFFFFFFu) == 257 && uc_spec_frames(156250, 0, 2048, 512) == 306);
  for (int i = 0; i < 20000; ++i) {
    const uint32_t fl = 1 + (uint32_t)(rng() % 2048), hop = 1 + (uint32_t)(rng() % (i % 2 ? 5000 : 0xFFFFFFFFull));
    const uint64_t n_in = 1 + rng() % (i % 3 ? 100000 : (1ull << 40));
    const int64_t first = (int64_t)(rng() % (n_in + fl - 1)) - (int64_t)(fl - 1);          // 1 - fl .. n_in - 1
    const int64_t got = uc_spec_frames(n_in, first, fl, hop);
    const __int128 span = (__int128)n_in - first;
    CHECK(got == (int64_t)((span + hop - 1) / hop) && got >= 1);
    CHECK((__int128)first + (__int128)(got - 1) * hop < (__int128)n_in && (__int128)first + (__int128)got * hop >= (__int128)n_in);
    ++counts;
  }
  const struct { uint64_t n_in; int64_t first; uint32_t fl, hop; } no_frames[] = {
      {0, 0, 4, 1}, {(1ull << 40) + 1, 0, 4, 1}, {~0ull, 0, 4, 1}, {10, 0, 0, 1}, {10, 0, 2049, 1}, {10, 0, 0xFFFFFFFFu, 1}, {10, 0, 4, 0},
      {10, -4, 4, 1}, {10, 10, 4, 1}, {10, std::numeric_limits<int64_t>::min(), 4, 1}, {10, std::numeric_limits<int64_t>::max(), 4, 1},
      {1ull << 40, (int64_t)(1ull << 40), 2048, 1}};
  for (const auto& c : no_frames) {
    CHECK(uc_spec_frames(c.n_in, c.first, c.fl, c.hop) == -EINVAL && strlen(uc_spec_last_error()) > 0);
    ++refused;
  }

  // ---- the plan
  for (int i = 0; i < 20000; ++i) {
    uc_spec_params p = defaults();
    p.frame_len = (uint32_t)(rng() % 2052);
    p.hop = (uint32_t)(rng() % 4000);
    p.bin_first = (uint32_t)(rng() % 1030);
    p.n_bins = (uint32_t)(rng() % 1030);
    p.kind = (int32_t)(rng() % 5) - 1;
    p.ac_bins = (uint32_t)(rng() % 2000);
    const uint64_t n_in = rng() % 20000;
    p.first = (int64_t)(rng() % 24000) - 2100;
    const size_t n_rows = (size_t)(rng() % 5), stride = rng() % 3 ? 0 : (size_t)(rng() % 1100);
    const bool frames_ok = n_in >= 1 && p.frame_len >= 1 && p.frame_len <= 2048 && p.hop >= 1 && p.first > -(int64_t)p.frame_len && p.first < (int64_t)n_in;
    const uint64_t frames = frames_ok ? (uint64_t)((n_in - p.first + p.hop - 1) / p.hop) : 0;
    p.n_frames = rng() % 4 ? 0 : rng() % (frames + 2);
    const bool ok = frames_ok && n_rows >= 1 && p.n_frames <= frames && p.n_bins >= 1 && p.bin_first + p.n_bins <= 1025 && (stride == 0 || stride >= p.n_bins) &&
                    p.kind >= 0 && p.kind <= 2;
    uc_spec_info f = {7, 7, 7, 7, 7};
    const int rc = uc_spec_plan(&p, n_rows, n_in, stride, &f);
    CHECK(rc == (ok ? 0 : -EINVAL));
    if (ok) {
      const uint64_t nf = p.n_frames ? p.n_frames : frames, os = stride ? stride : p.n_bins;
      CHECK(f.n_frames == nf && f.out_stride == os && f.out_elems == (n_rows * nf - 1) * os + p.n_bins && f.bin_first == p.bin_first && f.n_bins == p.n_bins);
      ++plans;
    } else {
      CHECK(f.n_frames == 7 && f.n_bins == 7 && strlen(uc_spec_last_error()) > 0);
      ++refused;
    }
  }
  {
    uc_spec_info f = {7, 7, 7, 7, 7};
    uc_spec_params p = defaults();
    CHECK(uc_spec_plan(nullptr, 1, 5000, 0, &f) == -EINVAL && uc_spec_plan(&p, 1, 5000, 0, nullptr) == -EINVAL);
    const float bad_floor[] = {0.0f, -0.0f, -1.0f, NAN, inf, -inf};
    for (float v : bad_floor) {
      p = defaults();
      p.floor = v;
      CHECK(uc_spec_plan(&p, 1, 5000, 0, &f) == -EINVAL);
      ++refused;
    }
    const float not_finite[] = {NAN, inf, -inf};
    for (float v : not_finite) {
      p = defaults();
      p.scale = v;
      CHECK(uc_spec_plan(&p, 1, 5000, 0, &f) == -EINVAL);
      p = defaults();
      p.db_mul = v;
      CHECK(uc_spec_plan(&p, 1, 5000, 0, &f) == -EINVAL);
      refused += 2;
    }
    p = defaults();
    p.reserved = 1;
    CHECK(uc_spec_plan(&p, 1, 5000, 0, &f) == -EINVAL);
    p = defaults();
    p.bin_first = 2;
    p.n_bins = 0xFFFFFFFFu;                                                // bin_first + n_bins wraps
    CHECK(uc_spec_plan(&p, 1, 5000, 0, &f) == -EINVAL);
    p = defaults();
    CHECK(uc_spec_plan(&p, (size_t)1 << 32, 5000, 0, &f) == -EINVAL && uc_spec_plan(&p, 1, 5000, (size_t)1 << 41, &f) == -EINVAL);
    p.frame_len = 1;
    p.hop = 1;                                                             // 2^40 frames a row
    CHECK(uc_spec_plan(&p, 2, (size_t)1 << 40, 0, &f) == -EINVAL && f.n_frames == 7);
    CHECK(uc_spec_plan(&p, 1, (size_t)1 << 40, 0, &f) == 0 && f.n_frames == (1ull << 40) && f.out_elems == ((1ull << 40) - 1) * 1025 + 1025);
    p = defaults();
    p.floor = std::numeric_limits<float>::denorm_min();
    p.scale = -0.0f;
    p.ac_bins = 0xFFFFFFFFu;
    p.first = -2047;
    CHECK(uc_spec_plan(&p, 0xFFFFFFFFu, 1, 0, &f) == 0 && f.n_frames == 1);
    refused += 7;
    plans += 2;
  }

  // ---- uc_spec_run: what is refused from the arguments alone.  `dev` is host memory: a call that passed every check before
  // the test for device memory is refused there (or, without a HIP runtime, at hipSetDevice), never run.
  std::vector<float> dev(8192);
  float* const o = dev.data() + 4096;
  uc_spec_peak* const pk = reinterpret_cast<uc_spec_peak*>(dev.data() + 6144);
  const uc_spec_params good = defaults();
  uc_spec_params hop0 = good, bins = good, kind = good, floor0 = good, first = good, frames = good;
  hop0.hop = 0;
  bins.bin_first = 1;
  kind.kind = 3;
  floor0.floor = 0.0f;
  first.first = 2048;
  frames.n_frames = 2;
  struct Case {
    const char* name;
    uc_spec* h;
    const void* in;
    int dtype;
    size_t n_rows, n_in, in_stride;
    const uc_spec_params* p;
    float* out;
    size_t out_stride;
    uc_spec_peak* peaks;
  };
  const Case cases[] = {
      {"spec NULL", nullptr, dev.data(), 1, 1, 2048, 0, &good, o, 0, nullptr},
      {"in NULL", fake(), nullptr, 1, 1, 2048, 0, &good, o, 0, nullptr},
      {"out NULL", fake(), dev.data(), 1, 1, 2048, 0, &good, nullptr, 0, nullptr},
      {"params NULL", fake(), dev.data(), 1, 1, 2048, 0, nullptr, o, 0, nullptr},
      {"dtype 2", fake(), dev.data(), 2, 1, 2048, 0, &good, o, 0, nullptr},
      {"dtype -1", fake(), dev.data(), -1, 1, 2048, 0, &good, o, 0, nullptr},
      {"no rows", fake(), dev.data(), 1, 0, 2048, 0, &good, o, 0, nullptr},
      {"too many rows", fake(), dev.data(), 1, (size_t)1 << 32, 2048, 0, &good, o, 0, nullptr},
      {"no samples", fake(), dev.data(), 1, 1, 0, 0, &good, o, 0, nullptr},
      {"n_in too large", fake(), dev.data(), 1, 1, ((size_t)1 << 40) + 1, 0, &good, o, 0, nullptr},
      {"in_stride < n_in", fake(), dev.data(), 1, 1, 2048, 2047, &good, o, 0, nullptr},
      {"in_stride too large", fake(), dev.data(), 1, 1, 2048, (size_t)1 << 41, &good, o, 0, nullptr},
      {"out_stride < n_bins", fake(), dev.data(), 1, 1, 2048, 0, &good, o, 1024, nullptr},
      {"out_stride too large", fake(), dev.data(), 1, 1, 2048, 0, &good, o, (size_t)1 << 41, nullptr},
      {"hop 0", fake(), dev.data(), 1, 1, 2048, 0, &hop0, o, 0, nullptr},
      {"bins beyond 1024", fake(), dev.data(), 1, 1, 2048, 0, &bins, o, 0, nullptr},
      {"kind 3", fake(), dev.data(), 1, 1, 2048, 0, &kind, o, 0, nullptr},
      {"floor 0", fake(), dev.data(), 1, 1, 2048, 0, &floor0, o, 0, nullptr},
      {"first = n_in", fake(), dev.data(), 1, 1, 2048, 0, &first, o, 0, nullptr},
      {"n_frames above the count", fake(), dev.data(), 1, 1, 2048, 0, &frames, o, 0, nullptr},
      {"out overlaps in", fake(), dev.data(), 1, 1, 2048, 0, &good, dev.data() + 2047, 0, nullptr},
      {"peaks overlap in", fake(), dev.data(), 1, 1, 2048, 0, &good, o, 0, reinterpret_cast<uc_spec_peak*>(dev.data() + 2046)},
      {"peaks overlap out", fake(), dev.data(), 1, 1, 2048, 0, &good, o, 0, reinterpret_cast<uc_spec_peak*>(o + 1024)},
      {"host memory", fake(), dev.data(), 1, 1, 2048, 0, &good, o, 0, pk},
  };
  for (const Case& c : cases) {
    const int rc = uc_spec_run(c.h, c.in, c.dtype, c.n_rows, c.n_in, c.in_stride, c.p, c.out, c.out_stride, c.peaks, nullptr);
    if (getenv("UC_SAN_TEXTS")) printf("%s: %d: %s\n", c.name, rc, uc_spec_last_error());   // to compare the texts of two builds
    const bool last = &c == &cases[sizeof(cases) / sizeof(cases[0]) - 1];                   // (-EIO where no HIP runtime answers)
    if ((rc != -EINVAL && !(last && rc == -EIO)) || strlen(uc_spec_last_error()) == 0) {
      printf("san_spec: %s: rc %d (%s)\n", c.name, rc, uc_spec_last_error());
      return 1;
    }
    ++refused;
  }

  // ---- uc_spec_set_window: refused before the object is read
  {
    std::vector<float> w(2048, 1.0f);
    CHECK(uc_spec_set_window(nullptr, w.data(), 2048) == -EINVAL && uc_spec_set_window(fake(), w.data(), 0) == -EINVAL);
    CHECK(uc_spec_set_window(fake(), w.data(), 2049) == -EINVAL && uc_spec_set_window(fake(), nullptr, 0) == -EINVAL);
    w[2047] = NAN;
    CHECK(uc_spec_set_window(fake(), w.data(), 2048) == -EINVAL);
    w[2047] = inf;
    CHECK(uc_spec_set_window(fake(), w.data(), 2048) == -EINVAL);
    refused += 6;
  }

  CHECK(uc_spec_abi_version() == UC_SPEC_ABI_VERSION);
  uc_spec* an = fake();
  CHECK(uc_spec_create(0, nullptr) == -EINVAL);
  uc_spec_destroy(nullptr);
  const int rc = uc_spec_create(0, &an);
  if (rc == 0) {
    // with a GPU the checks that need the object run too: host memory is no device memory
    CHECK(uc_spec_run(an, dev.data(), 1, 1, 2048, 0, &good, o, 0, nullptr, nullptr) == -EINVAL);
    uc_spec_destroy(an);
    printf("san_spec: %d frame counts, %d plans, %d refusals; a GPU is visible, uc_spec_create succeeded\n", counts, plans, refused);
  } else {
    CHECK(rc == -ENODEV && an == nullptr && strstr(uc_spec_last_error(), "no CPU path"));
    printf("san_spec: %d frame counts, %d plans, %d refusals; uc_spec_create: %d (%s)\n", counts, plans, refused, rc, uc_spec_last_error());
  }
  return 0;
}
