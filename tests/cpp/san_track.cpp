// san_track.cpp -- a stand-alone driver of the host translation unit of libuchirp_track.so (csrc/uc_track_api.cpp), built
// with AddressSanitizer and UndefinedBehaviorSanitizer by `make -C ultrasonic-communication_amd sanitize-track`:
// uc_track_finish on crafted records (empty, one slot, four slots, a tie, NOT_FINITE, slots out of range), each in a buffer
// of exactly its size; every refused argument of uc_track_windows that is decided before the object is touched; and --
// where a GPU is missing, as in the sanitizer's container -- the refusal of uc_track_create.  CPU only: it never launches a
// kernel.  With UC_SAN_TEXTS set it prints the library's last error text behind every check, so that two builds can be
// compared.
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "uchirp_track.h"

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      printf("san_track: %s failed (line %d)\n", #c, __LINE__);      \
      return 1;                                                      \
    }                                                                \
    if (getenv("UC_SAN_TEXTS")) printf("line %d: %s\n", __LINE__, uc_track_last_error()); \
  } while (0)

// a handle that is not NULL: every refusal below is decided from the arguments alone, before the object is used
static uc_track* fake() {
  static long long storage[128];
  return reinterpret_cast<uc_track*>(storage);
}

// one record on the heap, exactly its size: a read past it is a report
static std::unique_ptr<uc_track_crest> record() {
  std::unique_ptr<uc_track_crest> c(new uc_track_crest);
  memset(c.get(), 0, sizeof(uc_track_crest));
  for (int i = 0; i < UC_TRACK_SLOTS; ++i) c->slot[i].k = -1;
  return c;
}

static void put(uc_track_crest* c, int i, int k, double lo, double mid, double hi) {
  c->slot[i].k = k;
  c->slot[i].r[0] = lo;
  c->slot[i].r[1] = mid;
  c->slot[i].r[2] = hi;
}

int main() {
  std::unique_ptr<uc_track_peak_t> out(new uc_track_peak_t);
  int finished = 0;
  {  // empty: NO_PEAK, and AT_EDGE is carried over
    auto c = record();
    c->flags = UC_TRACK_NO_PEAK | UC_TRACK_AT_EDGE;
    CHECK(uc_track_finish(c.get(), 512, out.get()) == 0);
    CHECK(out->flags == (UC_TRACK_NO_PEAK | UC_TRACK_AT_EDGE) && out->delay_samples == 0.0 && out->height == 0.0 && out->runner_up == 0.0 && out->lag == 0);
    ++finished;
  }
  {  // one slot, symmetric: delay = lag, no runner-up
    auto c = record();
    c->n_candidates = 1;
    put(c.get(), 0, 2, 2.0, 3.0, 2.0);
    CHECK(uc_track_finish(c.get(), 2, out.get()) == 0);
    CHECK(out->flags == 0 && out->lag == 0 && out->delay_samples == 0.0 && out->height == 3.0 && out->runner_up == 0.0);
    ++finished;
  }
  {  // four slots: the third is the tallest, the first the runner-up; c outside (-1, 1) in the last
    auto c = record();
    c->n_candidates = 9;
    put(c.get(), 0, 1, 1.0, 8.0, 2.0);
    put(c.get(), 1, 40, 0.5, 4.0, 0.25);
    put(c.get(), 2, 700, 3.0, 10.0, 6.0);
    put(c.get(), 3, 1023, -9.0, 1.0, -9.0);
    CHECK(uc_track_finish(c.get(), 512, out.get()) == 0);
    CHECK(out->flags == 0 && out->lag == 700 - 512 && out->height >= 10.0 && out->delay_samples > 188.0 && out->delay_samples < 188.5);
    CHECK(out->runner_up > 0.79 && out->runner_up < 0.81);
    ++finished;
  }
  {  // an exact tie: the first one
    auto c = record();
    c->n_candidates = 2;
    put(c.get(), 0, 3, 0.0, 2.0, 0.0);
    put(c.get(), 1, 9, 0.0, 2.0, 0.0);
    CHECK(uc_track_finish(c.get(), 6, out.get()) == 0);
    CHECK(out->lag == 3 - 6 && out->runner_up == 1.0 && out->height == 2.0);
    ++finished;
  }
  {  // NOT_FINITE, slots out of range, bad arguments
    auto c = record();
    c->flags = UC_TRACK_NOT_FINITE;
    CHECK(uc_track_finish(c.get(), 512, out.get()) == -EINVAL && strlen(uc_track_last_error()) > 0);
    c->flags = 0;
    put(c.get(), 0, 0, 1.0, 2.0, 1.0);
    CHECK(uc_track_finish(c.get(), 512, out.get()) == -EINVAL);
    put(c.get(), 0, 1024, 1.0, 2.0, 1.0);
    CHECK(uc_track_finish(c.get(), 512, out.get()) == -EINVAL);
    put(c.get(), 0, -2, 1.0, 2.0, 1.0);
    CHECK(uc_track_finish(c.get(), 512, out.get()) == -EINVAL);
    put(c.get(), 0, 1023, 1.0, 2.0, 1.0);
    CHECK(uc_track_finish(c.get(), 512, out.get()) == 0);
    CHECK(uc_track_finish(c.get(), 511, out.get()) == -EINVAL);
    CHECK(uc_track_finish(nullptr, 512, out.get()) == -EINVAL && uc_track_finish(c.get(), 512, nullptr) == -EINVAL);
    CHECK(uc_track_finish(c.get(), 0, out.get()) == -EINVAL && uc_track_finish(c.get(), 513, out.get()) == -EINVAL);
    finished += 10;
  }

  // uc_track_windows: what is refused from the arguments alone.  `dev` is host memory: a call that passed every check before
  // the test for device memory is refused there (or, without a HIP runtime, at hipSetDevice), never run.
  std::vector<float> dev(4096);
  std::vector<uc_track_pair> pairs(2, uc_track_pair{0, 1});   // exactly two pairs: a read past them is a report
  std::vector<double> corr_mem(2 * 3 * 9 + 2 * 3 * 17);
  double* const co = corr_mem.data();
  uc_track_crest* const cr = reinterpret_cast<uc_track_crest*>(corr_mem.data() + 2 * 3 * 9);   // behind the correlations
  const size_t big = (size_t)1 << 41;
  struct Case {
    const char* name;
    uc_track* h;
    const void* in;
    int dtype;
    size_t n_mics, n_in, in_stride;
    const uc_track_pair* pr;
    size_t n_pairs, first, window_len, hop, n_windows;
    uint32_t L;
    double* corr;
    size_t corr_stride;
    uc_track_crest* crest;
  };
  const void* in = dev.data();
  const Case cases[] = {
      {"track NULL", nullptr, in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, co, 0, cr},
      {"in NULL", fake(), nullptr, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, co, 0, cr},
      {"both outputs NULL", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, nullptr, 0, nullptr},
      {"pairs NULL", fake(), in, 1, 2, 64, 0, nullptr, 2, 0, 16, 16, 3, 4, co, 0, cr},
      {"dtype 2", fake(), in, 2, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, co, 0, cr},
      {"dtype -1", fake(), in, -1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, co, 0, cr},
      {"no microphones", fake(), in, 1, 0, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, co, 0, cr},
      {"too many microphones", fake(), in, 1, (size_t)1 << 32, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, co, 0, cr},
      {"no pairs", fake(), in, 1, 2, 64, 0, pairs.data(), 0, 0, 16, 16, 3, 4, co, 0, cr},
      {"too many pairs", fake(), in, 1, 2, 64, 0, pairs.data(), (size_t)1 << 32, 0, 16, 16, 3, 4, co, 0, cr},
      {"no windows", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 0, 4, co, 0, cr},
      {"too many windows", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, (size_t)1 << 32, 4, co, 0, cr},
      {"pairs * windows too many", fake(), in, 1, 2, big / 2, 0, pairs.data(), 2, 0, 1, 1, (size_t)1 << 31, 4, nullptr, 0, cr},
      {"no input samples", fake(), in, 1, 2, 0, 0, pairs.data(), 2, 0, 16, 16, 3, 4, co, 0, cr},
      {"window_len 0", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 0, 16, 3, 4, co, 0, cr},
      {"hop 0", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 0, 3, 4, co, 0, cr},
      {"n_in too large", fake(), in, 1, 2, big, 0, pairs.data(), 2, 0, 16, 16, 3, 4, co, 0, cr},
      {"first > n_in", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 65, 16, 16, 1, 4, co, 0, cr},
      {"first + window_len > n_in", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 49, 16, 16, 1, 4, co, 0, cr},
      {"the last window past n_in", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 17, 16, 16, 3, 4, co, 0, cr},
      {"the last window past n_in, gaps", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 25, 3, 4, co, 0, cr},
      {"hop wraps", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, ~(size_t)0, 3, 4, co, 0, cr},
      {"max_lag 0", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 0, co, 0, cr},
      {"max_lag 513", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 513, co, 0, cr},
      {"in_stride < n_in", fake(), in, 1, 2, 64, 63, pairs.data(), 2, 0, 16, 16, 3, 4, co, 0, cr},
      {"corr_stride < lags", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, co, 8, cr},
      {"in_stride too large", fake(), in, 1, 2, 64, big, pairs.data(), 2, 0, 16, 16, 3, 4, co, 0, cr},
      {"corr_stride too large", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, co, big, cr},
      {"corr overlaps in", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, reinterpret_cast<double*>(dev.data() + 32), 0, cr},
      {"crest overlaps in", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, co, 0, reinterpret_cast<uc_track_crest*>(dev.data() + 126)},
      {"crest overlaps corr", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, co, 0, reinterpret_cast<uc_track_crest*>(co + 53)},
      {"crest overlaps strided corr", fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, co, 17, cr},
  };
  int refused = 0;
  for (const Case& c : cases) {
    const int rc = uc_track_windows(c.h, c.in, c.dtype, c.n_mics, c.n_in, c.in_stride, c.pr, c.n_pairs, c.first, c.window_len, c.hop,
                                    c.n_windows, c.L, c.corr, c.corr_stride, c.crest, nullptr);
    if (getenv("UC_SAN_TEXTS")) printf("%s: %d: %s\n", c.name, rc, uc_track_last_error());   // to compare the texts of two builds
    if (rc != -EINVAL || strlen(uc_track_last_error()) == 0) {
      printf("san_track: %s: rc %d (%s)\n", c.name, rc, uc_track_last_error());
      return 1;
    }
    ++refused;
  }
  // one bad pair at a time, the second of two
  const uc_track_pair bad[] = {{2, 0}, {0, 2}, {0xFFFFFFFFu, 0}};
  for (const uc_track_pair& b : bad) {
    pairs[1] = b;
    CHECK(uc_track_windows(fake(), in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, co, 0, cr, nullptr) == -EINVAL);
    CHECK(strstr(uc_track_last_error(), "pair 1"));
    ++refused;
  }
  pairs[1] = uc_track_pair{1, 1};

  CHECK(uc_track_abi_version() == UC_TRACK_ABI_VERSION);
  CHECK(uc_track_create(0, nullptr) == -EINVAL);
  uc_track_destroy(nullptr);
  uc_track* tr = nullptr;
  const int rc = uc_track_create(0, &tr);
  if (rc == 0) {
    // with a GPU the checks that need the object run too: host memory is no device memory
    CHECK(uc_track_windows(tr, in, 1, 2, 64, 0, pairs.data(), 2, 0, 16, 16, 3, 4, co, 0, cr, nullptr) == -EINVAL);
    uc_track_destroy(tr);
    printf("san_track: %d records finished or refused, %d refusals; a GPU is visible, uc_track_create succeeded\n", finished, refused);
  } else {
    CHECK(rc == -ENODEV && tr == nullptr && strstr(uc_track_last_error(), "no CPU path"));
    printf("san_track: %d records finished or refused, %d refusals; uc_track_create: %d (%s)\n", finished, refused, rc, uc_track_last_error());
  }
  return 0;
}
