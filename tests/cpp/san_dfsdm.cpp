// san_dfsdm.cpp -- a stand-alone driver of the host translation unit of libuchirp_dfsdm.so (csrc/uc_dfsdm_api.cpp), built with
// AddressSanitizer and UndefinedBehaviorSanitizer by `make -C ultrasonic-communication_amd sanitize-dfsdm`: the check at every
// limit of a configuration, the gain, the plan at the uint64 edges, one row of the filter against a restatement in 64-bit
// integers reduced to 32 bits -- from zero and from arbitrary states (every int32 sum may wrap: none may be undefined), all
// ones included, whole and cut into calls, into buffers of exactly their size --, every refused argument of
// uc_dfsdm_filter_row and of uc_dfsdm_run that is decided before the object is touched; and -- where a GPU is missing, as in
// the sanitizer's container -- the refusal of uc_dfsdm_create.  CPU only: it never launches a kernel.
// With UC_SAN_TEXTS set it prints the library's last error text behind every check, so that two builds can be compared.
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "uchirp_dfsdm.h"

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      printf("san_dfsdm: %s failed (line %d)\n", #c, __LINE__);      \
      return 1;                                                      \
    }                                                                \
    if (getenv("UC_SAN_TEXTS")) printf("line %d: %s\n", __LINE__, uc_dfsdm_last_error()); \
  } while (0)

// something that is not NULL for uc_dfsdm_create to overwrite.  (uc_dfsdm_run reads the object's configuration for the
// count of the outputs, so its refusals are driven with a real object, where a GPU lets one be made.)
struct FakeObject {
  long long storage[64];
};

static int32_t wrap(int64_t v) { return (int32_t)(uint32_t)(uint64_t)v; }

// the definition of uchirp_dfsdm.h in 64-bit integers, reduced to int32 after every sum
static size_t reference_row(const uc_dfsdm_config& c, const uint32_t* words, size_t n, uint64_t words_before, int32_t st[16], int32_t* out) {
  const int N = c.order == 0 ? 2 : c.order;
  uint64_t r = (32 * words_before) % c.ratio, i = ((32 * words_before) / c.ratio) % c.integrator;
  size_t k_out = 0;
  for (size_t j = 0; j < n; ++j)
    for (int b = 0; b < 32; ++b) {
      const int64_t s = (words[j] >> b) & 1u ? 1 : -1;
      st[0] = wrap((int64_t)st[0] + s);
      for (int k = 1; k < N; ++k) st[k] = wrap((int64_t)st[k] + st[k - 1]);
      if (++r < c.ratio) continue;
      r = 0;
      int32_t v = st[N - 1];
      for (int k = 0; k < N; ++k) {
        const int32_t d = wrap((int64_t)v - st[5 + k]);
        st[5 + k] = v;
        v = d;
      }
      if (c.order == 0) {
        const int32_t w = wrap((int64_t)v + st[11]);
        st[11] = st[10];
        st[10] = v;
        v = w;
      }
      st[12] = wrap((int64_t)st[12] + v);
      if (++i < c.integrator) continue;
      i = 0;
      int64_t y = ((int64_t)st[12] >> c.shift) - c.offset;
      st[12] = 0;
      y = y > 8388607 ? 8388607 : y < -8388608 ? -8388608 : y;
      out[k_out++] = (int32_t)(y * 256);
    }
  st[13] = st[14] = st[15] = 0;
  return k_out;
}

// (an empty vector's data() may be NULL, which memcmp must not be given)
static bool same(const int32_t* a, const int32_t* b, size_t n) { return n == 0 || memcmp(a, b, n * sizeof(int32_t)) == 0; }

int main() {
  std::mt19937_64 rng(27);
  int refused = 0, rows = 0;

  // ---- the check, the gain
  {
    const uc_dfsdm_config good[] = {{5, 32, 1, 2, 0}, {3, 32, 1, 2, 0}, {0, 16, 1, 0, 5}, {0, 1024, 1, 8, 0}, {1, 7, 3, 0, -3}, {1, 1, 1, 0, 0},
                                    {2, 64, 2, 0, 0}, {3, 20, 1, 0, 0}, {3, 5, 256, 0, 0}, {3, 1024, 1, 8, 0}, {4, 215, 1, 8, 0}, {5, 73, 1, 8, 100},
                                    {1, 1024, 256, 31, UC_DFSDM_OFFSET_MAX}, {5, 73, 1, 0, UC_DFSDM_OFFSET_MIN}};
    for (const auto& c : good) CHECK(uc_dfsdm_check(&c) == 0 && uc_dfsdm_gain(&c) >= 1 && uc_dfsdm_gain(&c) <= UC_DFSDM_GAIN_MAX);
    const uc_dfsdm_config sinc5 = {5, 73, 1, 0, 0}, sinc3 = {3, 1024, 2, 0, 0}, fast = {0, 1024, 1, 0, 0};
    CHECK(uc_dfsdm_gain(&sinc5) == 2073071593ull && uc_dfsdm_gain(&sinc3) == 2147483648ull && uc_dfsdm_gain(&fast) == 2097152ull);
    const uc_dfsdm_config bad[] = {{5, 74, 1, 0, 0}, {4, 216, 1, 0, 0}, {3, 1024, 2, 0, 0}, {6, 32, 1, 0, 0}, {-1, 32, 1, 0, 0}, {3, 0, 1, 0, 0},
                                   {1, 1025, 1, 0, 0}, {3, 32, 0, 0, 0}, {1, 32, 257, 0, 0}, {3, 32, 1, 32, 0}, {3, 32, 1, -1, 0},
                                   {3, 32, 1, 0, 8388608}, {3, 32, 1, 0, -8388609}, {5, 1024, 256, 0, 0}, {3, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0}};
    for (const auto& c : bad) {
      CHECK(uc_dfsdm_check(&c) == -EINVAL && strlen(uc_dfsdm_last_error()) > 0);
      ++refused;
    }
    CHECK(uc_dfsdm_check(nullptr) == -EINVAL && uc_dfsdm_gain(nullptr) == 0 && uc_dfsdm_gain(&bad[3]) == 0 && uc_dfsdm_gain(&bad[5]) == 0);
    ++refused;
  }

  // ---- the plan, at the edges of its range
  {
    const uc_dfsdm_config c = {3, 20, 1, 0, 0}, one = {1, 1, 1, 0, 0}, slow = {1, 1024, 256, 0, 0};
    const uint64_t top = (uint64_t)1 << 58;
    uint64_t n = 7;
    CHECK(uc_dfsdm_plan(&c, 0, 5, &n) == 0 && n == 8);
    CHECK(uc_dfsdm_plan(&c, 5, 0, &n) == 0 && n == 0);
    CHECK(uc_dfsdm_plan(&one, top - 3, 3, &n) == 0 && n == 96);
    CHECK(uc_dfsdm_plan(&one, 0, top, &n) == 0 && n == 32 * top);
    CHECK(uc_dfsdm_plan(&slow, top - 8192, 8192, &n) == 0 && n == 1);
    uint64_t sum = 0, at = 0;
    for (uint64_t k : {1u, 16u, 17u, 33u}) {
      CHECK(uc_dfsdm_plan(&c, at, k, &n) == 0);
      sum += n;
      at += k;
    }
    CHECK(uc_dfsdm_plan(&c, 0, 67, &n) == 0 && n == sum && n == 107);
    CHECK(uc_dfsdm_plan(&c, 0, 5, nullptr) == -EINVAL && uc_dfsdm_plan(nullptr, 0, 5, &n) == -EINVAL);
    CHECK(uc_dfsdm_plan(&c, top, 1, &n) == -EINVAL && uc_dfsdm_plan(&c, 1, top, &n) == -EINVAL && uc_dfsdm_plan(&c, ~(uint64_t)0, ~(uint64_t)0, &n) == -EINVAL);
    refused += 5;
  }

  // ---- one row of the filter
  {
    const uc_dfsdm_config cfgs[] = {{5, 32, 1, 2, 0}, {3, 32, 1, 0, 0}, {0, 16, 1, 0, 5}, {0, 1024, 1, 8, 0}, {1, 7, 3, 0, -3}, {1, 1, 1, 0, 0},
                                    {2, 64, 2, 0, 0}, {3, 20, 1, 0, 0}, {3, 5, 256, 0, 0}, {3, 1024, 1, 8, 0}, {4, 215, 1, 8, 0}, {5, 73, 1, 8, 100},
                                    {3, 64, 3, 0, 0}, {5, 73, 1, 0, UC_DFSDM_OFFSET_MIN}, {1, 3, 1, 31, UC_DFSDM_OFFSET_MAX}};
    int k = 0;
    for (const auto& c : cfgs)
      for (int kind = 0; kind < 4; ++kind, ++k) {
        const size_t n = 1 + (size_t)(rng() % 150);
        const uint64_t wb = kind == 0 ? 0 : rng() % 100000;
        std::vector<uint32_t> w(n);
        for (auto& v : w) v = kind == 1 ? 0xFFFFFFFFu : kind == 2 ? 0u : (uint32_t)rng();
        int32_t s0[16] = {0};
        if (kind == 3)
          for (int i = 0; i < 16; ++i) s0[i] = (int32_t)(uint32_t)rng();
        uint64_t planned = 0;
        CHECK(uc_dfsdm_plan(&c, wb, n, &planned) == 0);
        // buffers of exactly the planned size: a word too many is the sanitizer's to find
        std::vector<int32_t> oa(32 * n), ob(planned), oc(planned);
        int32_t a[16], b[16], cc[16];
        memcpy(a, s0, sizeof(a));
        memcpy(b, s0, sizeof(b));
        memcpy(cc, s0, sizeof(cc));
        const size_t na = reference_row(c, w.data(), n, wb, a, oa.data());
        size_t nb = 99, n1 = 0, n2 = 0;
        CHECK(na == planned);
        CHECK(uc_dfsdm_filter_row(&c, w.data(), n, wb, b, ob.data(), ob.size(), &nb) == 0 && nb == planned);
        CHECK(same(oa.data(), ob.data(), planned));
        // the words the order does not use stay; the reserved ones are written 0 by both
        CHECK(memcmp(a, b, sizeof(a)) == 0);
        const size_t cut = (size_t)(rng() % n);                  // 0: one call
        if (cut) CHECK(uc_dfsdm_filter_row(&c, w.data(), cut, wb, cc, oc.data(), oc.size(), &n1) == 0);
        CHECK(uc_dfsdm_filter_row(&c, w.data() + cut, n - cut, wb + cut, cc, oc.data() + n1, oc.size() - n1, &n2) == 0 && n1 + n2 == planned);
        CHECK(same(oa.data(), oc.data(), planned) && memcmp(a, cc, sizeof(a)) == 0);
        ++rows;
      }
    const uc_dfsdm_config c = {3, 32, 1, 2, 0};
    uint32_t w[4] = {1, 2, 3, 4};
    int32_t st[16] = {0}, out[4] = {7, 7, 7, 7};
    size_t n = 0;
    CHECK(uc_dfsdm_filter_row(nullptr, w, 4, 0, st, out, 4, &n) == -EINVAL && uc_dfsdm_filter_row(&c, nullptr, 4, 0, st, out, 4, &n) == -EINVAL);
    CHECK(uc_dfsdm_filter_row(&c, w, 4, 0, nullptr, out, 4, &n) == -EINVAL && uc_dfsdm_filter_row(&c, w, 4, 0, st, nullptr, 4, &n) == -EINVAL);
    CHECK(uc_dfsdm_filter_row(&c, w, 4, 0, st, out, 4, nullptr) == -EINVAL && uc_dfsdm_filter_row(&c, w, 0, 0, st, out, 4, &n) == -EINVAL);
    CHECK(uc_dfsdm_filter_row(&c, w, 4, 0, st, out, 3, &n) == -EINVAL && uc_dfsdm_filter_row(&c, w, 4, (uint64_t)1 << 58, st, out, 4, &n) == -EINVAL);
    for (int i = 0; i < 16; ++i) CHECK(st[i] == 0);
    for (int i = 0; i < 4; ++i) CHECK(out[i] == 7);
    // a call without outputs needs no output buffer
    const uc_dfsdm_config slow = {3, 1024, 1, 8, 0};
    CHECK(uc_dfsdm_filter_row(&slow, w, 4, 0, st, nullptr, 0, &n) == 0 && n == 0 && st[0] != 0);
    refused += 8;
  }

  // ---- create, and uc_dfsdm_run: what is refused from the arguments alone.  `dev` is host memory: a call that passed every
  // check before the test for device memory is refused there, never run.
  uc_dfsdm* obj = nullptr;
  const uc_dfsdm_config cfg = {3, 32, 1, 2, 0};
  CHECK(uc_dfsdm_create(0, &cfg, nullptr) == -EINVAL);
  CHECK(uc_dfsdm_create(0, nullptr, &obj) == -EINVAL && obj == nullptr);
  const uc_dfsdm_config bad_cfgs[] = {{5, 74, 1, 0, 0}, {3, 1024, 2, 0, 0}, {6, 32, 1, 0, 0}, {3, 32, 1, 32, 0}};
  for (const auto& c : bad_cfgs) {
    static FakeObject fake;
    obj = reinterpret_cast<uc_dfsdm*>(&fake);
    CHECK(uc_dfsdm_create(0, &c, &obj) == -EINVAL && obj == nullptr);      // a refused configuration is refused with or without a GPU
    ++refused;
  }
  uc_dfsdm_destroy(nullptr);
  alignas(16) static uint32_t dev[512];
  int32_t* const st = (int32_t*)(dev + 256);
  int32_t* const o = (int32_t*)(dev + 64);
  CHECK(uc_dfsdm_run(nullptr, dev, 2, 16, 0, 0, st, o, 0, nullptr) == -EINVAL);
  ++refused;
  const int rc = uc_dfsdm_create(0, &cfg, &obj);
  if (rc == 0) {
    const size_t big = ((size_t)1 << 40) + 1;
    struct Case {
      const char* name;
      const uint32_t* in;
      size_t n_rows, n, in_stride;
      uint64_t wb;
      int32_t* state;
      int32_t* out;
      size_t out_stride;
    };
    const Case cases[] = {
        {"pdm NULL", nullptr, 2, 16, 0, 0, st, o, 0},
        {"state NULL", dev, 2, 16, 0, 0, nullptr, o, 0},
        {"out NULL", dev, 2, 16, 0, 0, st, nullptr, 0},
        {"no rows", dev, 0, 16, 0, 0, st, o, 0},
        {"too many rows", dev, (size_t)1 << 32, 16, 0, 0, st, o, 0},
        {"no words", dev, 2, 0, 0, 0, st, o, 0},
        {"words_before too large", dev, 2, 16, 0, (uint64_t)1 << 58, st, o, 0},
        {"in_stride < n_words", dev, 2, 16, 15, 0, st, o, 0},
        {"out_stride < n_out", dev, 2, 16, 0, 0, st, o, 15},
        {"in_stride too large", dev, 2, 16, big, 0, st, o, 0},
        {"out_stride too large", dev, 2, 16, 0, 0, st, o, big},
        {"n_words too large", dev, 2, big, 0, 0, st, o, 0},
        {"pdm not on 4 bytes", (const uint32_t*)((const char*)dev + 2), 2, 16, 0, 0, st, o, 0},
        {"out not on 4 bytes", dev, 2, 16, 0, 0, st, (int32_t*)((char*)o + 1), 0},
        {"state not on 4 bytes", dev, 2, 16, 0, 0, (int32_t*)((char*)st + 2), o, 0},
        {"out overlaps pdm", dev, 2, 16, 0, 0, st, (int32_t*)dev + 31, 0},
        {"pdm overlaps out", dev + 95, 2, 16, 0, 0, st, o, 0},
        {"state overlaps pdm", dev, 2, 16, 0, 0, (int32_t*)(dev + 31), o, 0},
        {"state overlaps out", dev, 2, 16, 0, 0, (int32_t*)(o + 31), o, 0},
        {"out overlaps state", dev, 2, 16, 0, 0, st, st + 31, 0},
        {"host memory", dev, 2, 16, 0, 0, st, o, 0},
    };
    for (const Case& c : cases) {
      const int r = uc_dfsdm_run(obj, c.in, c.n_rows, c.n, c.in_stride, c.wb, c.state, c.out, c.out_stride, nullptr);
      if (getenv("UC_SAN_TEXTS")) printf("%s: %d: %s\n", c.name, r, uc_dfsdm_last_error());
      if (r != -EINVAL || strlen(uc_dfsdm_last_error()) == 0) {
        printf("san_dfsdm: %s: rc %d (%s)\n", c.name, r, uc_dfsdm_last_error());
        return 1;
      }
      ++refused;
    }
    uc_dfsdm_destroy(obj);
    printf("san_dfsdm: %d rows, %d refusals; a GPU is visible, uc_dfsdm_create succeeded\n", rows, refused);
  } else {
    CHECK(rc == -ENODEV && obj == nullptr && strstr(uc_dfsdm_last_error(), "no CPU path"));
    printf("san_dfsdm: %d rows, %d refusals; uc_dfsdm_create: %d (%s)\n", rows, refused, rc, uc_dfsdm_last_error());
  }
  return 0;
}
