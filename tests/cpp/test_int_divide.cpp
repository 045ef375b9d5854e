// Host check of csrc/int_divide.hpp: the magic-number quotient the integer Bilinear kernels use equals truncating
// division (C++ `/`, which truncates toward zero like Rust's) -- every i32 divisor up to 2^16 against edge
// numerators, random pairs for i32 and i64.  Prints "ok <checks>" and exits 0, or the first mismatch and exits 1.
#include <cstdio>
#include <cstdint>
#include <limits>
#include <random>
#include <vector>

#include "int_divide.hpp"

template <class T>
static bool check(T n, T d, unsigned long long& count) {
  const ndi::IntMagic<T> mg = ndi::int_magic<T>(d);
  const T got = ndi::int_div_magic<T>(n, mg), want = n / d;
  ++count;
  if (got != want) {
    std::printf("MISMATCH %d-bit: %lld / %lld = %lld, magic gives %lld\n", (int)(8 * sizeof(T)), (long long)n,
                (long long)d, (long long)want, (long long)got);
    return false;
  }
  return true;
}

template <class T>
static std::vector<T> edges(T d) {
  const T lo = std::numeric_limits<T>::min(), hi = std::numeric_limits<T>::max();
  std::vector<T> v = {lo, (T)(lo + 1), (T)-1, 0, 1, hi, (T)(hi - 1)};
  for (T k : {(T)1, (T)2, (T)3, (T)1000, (T)(hi / d)}) {
    if (k > hi / d) continue;
    const T m = (T)(k * d);
    for (T s : {(T)1, (T)-1}) {
      const T b = (T)(s * m);
      v.push_back(b);
      if (b < hi) v.push_back((T)(b + 1));
      if (b > lo) v.push_back((T)(b - 1));
    }
  }
  return v;
}

int main() {
  unsigned long long count = 0;
  for (int32_t d = 1; d <= (1 << 16); ++d)
    for (int32_t n : edges<int32_t>(d))
      if (!check<int32_t>(n, d, count)) return 1;
  std::mt19937_64 rng(12345);
  for (int i = 0; i < 2000000; ++i) {
    const int32_t n = (int32_t)rng();
    int32_t d = (int32_t)(rng() & 0x7fffffffu) >> (rng() % 31);
    if (d < 1) d = 1;
    if (!check<int32_t>(n, d, count)) return 1;
  }
  const int64_t big[] = {1, 2, 3, 5, 7, 10, 641, 65537, (int64_t)1 << 31, ((int64_t)1 << 32) + 1, 1000000007,
                         ((int64_t)1 << 62) - 1, (int64_t)1 << 62, std::numeric_limits<int64_t>::max()};
  for (int64_t d : big)
    for (int64_t n : edges<int64_t>(d))
      if (!check<int64_t>(n, d, count)) return 1;
  for (int64_t d = 1; d <= 4096; ++d)
    for (int64_t n : edges<int64_t>(d))
      if (!check<int64_t>(n, d, count)) return 1;
  for (int i = 0; i < 2000000; ++i) {
    const int64_t n = (int64_t)rng();
    int64_t d = (int64_t)(rng() >> 1) >> (rng() % 63);
    if (d < 1) d = 1;
    if (!check<int64_t>(n, d, count)) return 1;
  }
  std::printf("ok %llu\n", count);
  return 0;
}
