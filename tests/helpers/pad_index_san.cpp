// AddressSanitizer + UBSan harness over the pad index map (csrc/pad_index.h) as plain host C++: every pad type on the
// exhaustive small grid of tests/test_pad_index.py, each index used to read a signal of exactly n samples, plus far
// positions through the reciprocal branch of pad_fold.  Built and run on the CPU by tests/test_pad_index.py.
// Exit code 0 = no sanitizer report and the self-checks hold.
#include <cstdio>
#include <vector>

#include "../../ssqueeze_rs_amd/csrc/pad_index.h"

using namespace ssq;

static int fails = 0;
#define CHECK(c)                                          \
  do {                                                    \
    if (!(c)) {                                           \
      std::fprintf(stderr, "check failed: %s\n", #c);     \
      ++fails;                                            \
    }                                                     \
  } while (0)

static long long mod(long long m, long long p) { return ((m % p) + p) % p; }

static long long expect(int code, long long m, long long n) {
  const bool in = m >= 0 && m < n;
  switch (code) {
    case PAD_REFLECT: {
      const long long mm = m < 0 ? -m : 2 * n - 2 - m;
      return in ? m : (mm >= 0 && mm < n ? mm : -1);
    }
    case PAD_SYMMETRIC: {
      const long long r = mod(m, 2 * n);
      return r < n ? r : 2 * n - 1 - r;
    }
    case PAD_REPLICATE: return m < 0 ? 0 : (m >= n ? n - 1 : m);
    case PAD_WRAP: return mod(m, n);
    default: return in ? m : -1;
  }
}

int main() {
  for (int code = 0; code <= 5; ++code)
    for (long long n = 1; n <= 9; ++n) {
      std::vector<double> x((size_t)n);                    // heap block of exactly n samples: a stray index is a report
      for (long long i = 0; i < n; ++i) x[(size_t)i] = (double)i;
      for (long long m = -3 * n - 2; m <= 4 * n + 2; ++m) {
        const long long idx = pad_index(code, m, n);
        CHECK(idx == expect(code, m, n));
        CHECK(idx >= -1 && idx < n);
        if (idx >= 0) CHECK(x.data()[idx] == (double)idx);
      }
    }
  for (long long n : {1LL, 2LL, 7LL, 1000LL, (1LL << 31) + 5})
    for (long long m : {-(1LL << 45) - 3, -(1LL << 40), -1000 * n, -5 * n - 1, -5 * n, 5 * n - 1, 5 * n, 1000 * n + 3,
                        (1LL << 45) + 11})
      for (int code = 0; code <= 4; ++code) CHECK(pad_index(code, m, n) == expect(code, m, n));
  std::printf(fails ? "FAILED\n" : "ok\n");
  return fails ? 1 : 0;
}
