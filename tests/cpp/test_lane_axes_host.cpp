// The column validation of an x axis per lane (csrc/host_logic.hpp: first_bad_lane_axis, check_lane_axes), stand-alone:
// compiled with -fsanitize=address,undefined by tests/test_lane_axes_abi.py.  The tables are heap allocations of exactly
// n * lanes elements, so a read past either end is reported.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../ndarray-interp_amd/csrc/host_logic.hpp"

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

template <class T>
static std::vector<T> rising(uint64_t n, uint64_t lanes) {
  std::vector<T> x(n * lanes);
  for (uint64_t i = 0; i < n; ++i)
    for (uint64_t l = 0; l < lanes; ++l) x[i * lanes + l] = T(i) * T(l + 1) + T(l) * T(0.25);
  return x;
}

template <class T>
static void run() {
  const T nan = std::numeric_limits<T>::quiet_NaN(), inf = std::numeric_limits<T>::infinity();
  for (uint64_t n : {2ull, 3ull, 5ull, 33ull})
    for (uint64_t lanes : {1ull, 3ull, 65ull}) {
      const std::vector<T> x = rising<T>(n, lanes);
      CHECK(ndi::first_bad_lane_axis(x.data(), n, lanes) == lanes);
      CHECK(ndi::check_lane_axes(x.data(), n, lanes, NDI_LINEAR) == NDI_OK);
      for (uint64_t lane : {lanes - 1, lanes / 2, (uint64_t)0}) {
        std::vector<T> t = x;                       // a tie between the last two knots
        t[(n - 1) * lanes + lane] = t[(n - 2) * lanes + lane];
        CHECK(ndi::first_bad_lane_axis(t.data(), n, lanes) == lane);
        std::vector<T> f = x;                       // a fall at the first pair
        f[lane] = f[lanes + lane] + T(1);
        CHECK(ndi::first_bad_lane_axis(f.data(), n, lanes) == lane);
        for (uint64_t row : {(uint64_t)0, n / 2, n - 1}) {   // a NaN anywhere in the column, the ends included
          std::vector<T> v = x;
          v[row * lanes + lane] = nan;
          CHECK(ndi::first_bad_lane_axis(v.data(), n, lanes) == lane);
          CHECK(ndi::check_lane_axes(v.data(), n, lanes, NDI_LINEAR) == NDI_MONOTONIC);
          CHECK(ndi::tls_error() == "Values in the x axis need to be strictly monotonic rising (lane " + std::to_string(lane) + ")");
        }
      }
      if (lanes >= 3) {   // two offenders: the lowest lane is named, wherever its pair lies
        std::vector<T> v = x;
        v[(n - 1) * lanes + 1] = v[(n - 2) * lanes + 1];
        v[lanes + 2] = v[2];
        CHECK(ndi::first_bad_lane_axis(v.data(), n, lanes) == 1);
      }
      std::vector<T> e = x;   // infinite end knots are ordered like any others
      e[0] = -inf;
      e[(n - 1) * lanes + lanes - 1] = inf;
      CHECK(ndi::first_bad_lane_axis(e.data(), n, lanes) == lanes);
    }
  // the strategy's minimum length comes before the columns
  const std::vector<T> two = rising<T>(2, 4);
  CHECK(ndi::check_lane_axes(two.data(), 2, 4, NDI_PCHIP) == NDI_OK);
  CHECK(ndi::check_lane_axes(two.data(), 2, 4, NDI_CUBIC_HERMITE) == NDI_OK);
  CHECK(ndi::check_lane_axes(two.data(), 2, 4, NDI_CUBIC_SPLINE) == NDI_NOT_ENOUGH_DATA);
  CHECK(ndi::check_lane_axes(two.data(), 2, 4, NDI_AKIMA) == NDI_NOT_ENOUGH_DATA);
  std::vector<T> one(4, nan);
  CHECK(ndi::check_lane_axes(one.data(), 1, 4, NDI_LINEAR) == NDI_NOT_ENOUGH_DATA);
}

int main() {
  run<float>();
  run<double>();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
