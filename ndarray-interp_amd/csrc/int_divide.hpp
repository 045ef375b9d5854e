// csrc/int_divide.hpp -- signed integer division by an invariant positive divisor (Granlund-Montgomery, "Division
// by invariant integers using multiplication", PLDI 1994; the signed form of Hacker's Delight 10-4).
//
// The integer Bilinear's y step divides by dy = y[yi+1] - y[yi] (bilinear.rs:96 through linear.rs:33), which depends
// only on the y interval: its magic multiplier is formed once at create time and every division in the hot path
// becomes a high multiply, an add, a shift and a sign fix -- integer division is a long emulated sequence on CDNA.
// The quotient truncates toward zero, exactly as Rust's `i32 / i32` and `i64 / i64` do.
//
// Plain C++ for the host (the magic numbers are formed there; tests/cpp/test_int_divide.cpp checks the quotient
// against `/` on the host) and HIP for the device: the same source serves both.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NDI_HD __host__ __device__
#else
#define NDI_HD
#endif

namespace ndi {

template <class T>
struct IntMagic {
  T mult;       // the multiplier, read as a signed number of T's width
  int32_t shift;
  int32_t one;  // divisor 1: the quotient is the numerator (no multiplier of T's width exists for it)
};

template <class T> struct IntTraits;
template <> struct IntTraits<int32_t> { typedef uint32_t U; static constexpr int W = 32; };
template <> struct IntTraits<int64_t> { typedef uint64_t U; static constexpr int W = 64; };

// Magic numbers for a divisor d >= 1 (Hacker's Delight, figure 10-1, restricted to positive divisors).
template <class T>
inline IntMagic<T> int_magic(T d) {
  typedef typename IntTraits<T>::U U;
  constexpr int W = IntTraits<T>::W;
  IntMagic<T> mg{0, 0, 0};
  if (d == 1) {
    mg.one = 1;
    return mg;
  }
  const U two = (U)1 << (W - 1);
  const U ad = (U)d;
  const U anc = two - 1 - two % ad;  // |nc|: the largest numerator with nc % ad == ad - 1
  int p = W - 1;
  U q1 = two / anc, r1 = two - q1 * anc;
  U q2 = two / ad, r2 = two - q2 * ad;
  U delta;
  do {
    ++p;
    q1 *= 2; r1 *= 2;
    if (r1 >= anc) { ++q1; r1 -= anc; }
    q2 *= 2; r2 *= 2;
    if (r2 >= ad) { ++q2; r2 -= ad; }
    delta = ad - r2;
  } while (q1 < delta || (q1 == delta && r1 == 0));
  mg.mult = (T)(q2 + 1);
  mg.shift = p - W;
  return mg;
}

NDI_HD inline int32_t int_mulhi(int32_t a, int32_t b) { return (int32_t)(((int64_t)a * (int64_t)b) >> 32); }
NDI_HD inline int64_t int_mulhi(int64_t a, int64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __mul64hi(a, b);
#else
  return (int64_t)(((__int128)a * (__int128)b) >> 64);
#endif
}

// n / d, truncated toward zero, for the d int_magic was formed for.
template <class T>
NDI_HD inline T int_div_magic(T n, const IntMagic<T>& mg) {
  typedef typename IntTraits<T>::U U;
  constexpr int W = IntTraits<T>::W;
  if (mg.one) return n;
  T q = int_mulhi(mg.mult, n);
  if (mg.mult < 0) q = (T)((U)q + (U)n);   // the multiplier is >= 2^(W-1): add the numerator back
  q = q >> mg.shift;                        // arithmetic shift (floor)
  return (T)((U)q + ((U)n >> (W - 1)));     // floor -> toward zero for a negative numerator
}

}  // namespace ndi
