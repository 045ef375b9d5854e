// csrc/int_kernels.hpp -- the i32 / i64 Linear and Bilinear kernels (included by kernels.hpp).
//
// The reference's Linear and Bilinear are generic over `T: Num + PartialOrd + ...` (linear.rs:13-36,
// bilinear.rs:20-27, 64-99): for integer T, linear.rs:33's m = (y2 - y1) / (x2 - x1) truncates toward zero and every
// intermediate must fit T (a Rust debug build panics "attempt to {subtract,multiply,add,divide} with overflow").
// These kernels reproduce that exactly:
//   int_slopes1d_kernel / int_slopes2d_kernel
//                          create time: slope records {y, m} per knot and lane (m = 0 on the last knot), so the hot
//                          path has no integer division; intervals whose dy / dx (or division) overflow are marked.
//                          1-D also reduces, per interval, the set of d = x - x1 for which m * d and m * d + y1 fit T
//                          in every lane: each lane's set is an interval, so their intersection [lo, hi] is one too
//                          (exact ceil / floor divisions) -- a query then fails iff x - x1 overflows or leaves [lo, hi].
//   int_check1d_kernel     1-D first-error pre-pass for caller-owned buffers: reads the queries, the knots and 16 B per
//                          interval, never the records (as cheap as the float range pre-pass)
//   int_eval1d_kernel      1-D evaluation, m * d + y1 in T; FLAT: one output element per thread (short rows, scalar
//                          data: query per lane), WAVE: one query per wavefront, a lane per trailing element (long rows)
//   int_eval2d_kernel      2-D evaluation: the x step from the point records {z, m_x} at (xi, yi) and (xi, yi + 1) (one
//                          contiguous run per query), the y step's division by dy through the y interval's magic
//                          multiplier (int_divide.hpp); every operation is overflow-checked per lane.  CHECK / WRITE
//                          select the fused form (both), the write-free first-error pass (CHECK) and the rows before
//                          the first failure (WRITE)
// The kernels report only "some query failed" (the lowest flat index, atomicMin); which operation of which lane failed
// first is found for that one query on the host afterwards (int_host.hpp, IntEngine::diagnose / diagnose_at).
#pragma once
#include "int_divide.hpp"

namespace ndi {

template <class T>
struct IntRec {   // slope record: the value at the knot / grid point and the slope towards the next knot in x
  T v, m;
};
struct IntIv {    // admissible d = x - x1 of a 1-D interval (every lane's m * d and m * d + y1 fit T); empty: lo > hi
  long long lo, hi;
};
template <class T>
struct IntYIv {   // 2-D y interval: dy = y[yi+1] - y[yi] and its magic multiplier; bad: dy overflows T
  IntMagic<T> mg;
  T dy;
  int32_t bad;
};

template <class T>
__device__ __forceinline__ T wrap_mad(T m, T d, T v) {   // m * d + v in T, wrapping (only used where it cannot overflow)
  typedef typename IntTraits<T>::U U;
  return (T)((U)m * (U)d + (U)v);
}

// VectorExtensions::get_lower_index for integer knots: the unique i with k[i] <= x < k[i+1], clamped to [0, n-2]
// (generic_host.lower_index; the reference's O(1) first guess is not reproduced).
template <class T>
__device__ __forceinline__ uint32_t int_lower_index(const T* k, uint32_t n, T x) {
  if (x <= k[0]) return 0;
  if (x >= k[n - 1]) return n - 2;
  uint32_t lo = 0, hi = n - 1;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (k[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Exact floor / ceil of a / b (b != 0, the quotient representable).
__device__ __forceinline__ long long floor_div(long long a, long long b) {
  long long q = a / b;
  if ((a % b != 0) && ((a < 0) != (b < 0))) --q;
  return q;
}
__device__ __forceinline__ long long ceil_div(long long a, long long b) {
  long long q = a / b;
  if ((a % b != 0) && ((a < 0) == (b < 0))) ++q;
  return q;
}

// The set of d in T with m * d and m * d + y1 both in T (y1 in T): m * d in [A, B], A <= 0 <= B.
template <class T>
__device__ __forceinline__ void int_d_range(T m, T y1, long long& lo, long long& hi) {
  const long long tmin = (long long)(T)((typename IntTraits<T>::U)1 << (IntTraits<T>::W - 1));
  const long long tmax = (long long)(T)(((typename IntTraits<T>::U)1 << (IntTraits<T>::W - 1)) - 1);
  const long long A = y1 > 0 ? tmin : tmin - (long long)y1;
  const long long B = y1 < 0 ? tmax : tmax - (long long)y1;
  if (m == 0) {
    lo = tmin;
    hi = tmax;
  } else if (m == -1) {              // B / -1 and A / -1 without the i64 MIN / -1 overflow
    lo = -B;
    hi = A == tmin ? tmax : -A;
  } else if (m > 0) {
    lo = ceil_div(A, (long long)m);
    hi = floor_div(B, (long long)m);
  } else {
    lo = ceil_div(B, (long long)m);
    hi = floor_div(A, (long long)m);
  }
}

// Create time, 1-D: rec[i][l] = {y[i][l], (y[i+1][l] - y[i][l]) / (x[i+1] - x[i])}; iv[i] starts as the whole of T and
// is narrowed by every lane (atomicMax / atomicMin); an overflowing dy / dx / division empties it.
template <class T>
__global__ __launch_bounds__(BLOCK) void int_slopes1d_kernel(const T* __restrict__ x, const T* __restrict__ y,
                                                             uint64_t n, uint64_t lanes, IntRec<T>* __restrict__ rec,
                                                             IntIv* __restrict__ iv) {
  const uint64_t total = n * lanes;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (uint64_t)gridDim.x * BLOCK) {
    const uint64_t i = e / lanes;
    const T y1 = y[e];
    if (i + 1 >= n) {
      rec[e] = IntRec<T>{y1, (T)0};
      continue;
    }
    const T y2 = y[e + lanes];
    T dy, dx, m = 0;
    bool bad = __builtin_sub_overflow(y2, y1, &dy);
    bad |= __builtin_sub_overflow(x[i + 1], x[i], &dx);
    if (!bad) {
      if (dx == 0 || (dx == (T)-1 && dy == (T)((typename IntTraits<T>::U)1 << (IntTraits<T>::W - 1)))) bad = true;
      else m = dy / dx;
    }
    rec[e] = IntRec<T>{y1, m};
    if (bad) {
      atomicMax(&iv[i].lo, 1ll);
      atomicMin(&iv[i].hi, 0ll);
    } else {
      long long lo, hi;
      int_d_range<T>(m, y1, lo, hi);
      atomicMax(&iv[i].lo, lo);
      atomicMin(&iv[i].hi, hi);
    }
  }
}

// Create time, 2-D: rec[xi][yi][l] = {z, (z[xi+1][yi][l] - z[xi][yi][l]) / (x[xi+1] - x[xi])}; pbad[xi][yi] = 1 where a
// lane's dz / dx / division overflows.
template <class T>
__global__ __launch_bounds__(BLOCK) void int_slopes2d_kernel(const T* __restrict__ x, const T* __restrict__ z,
                                                             uint64_t nx, uint64_t ny, uint64_t lanes,
                                                             IntRec<T>* __restrict__ rec, uint8_t* __restrict__ pbad) {
  const uint64_t row = ny * lanes, total = nx * row;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (uint64_t)gridDim.x * BLOCK) {
    const uint64_t xi = e / row;
    const T z1 = z[e];
    if (xi + 1 >= nx) {
      rec[e] = IntRec<T>{z1, (T)0};
      continue;
    }
    T dz, dx, m = 0;
    bool bad = __builtin_sub_overflow(z[e + row], z1, &dz);
    bad |= __builtin_sub_overflow(x[xi + 1], x[xi], &dx);
    if (!bad) {
      if (dx == 0 || (dx == (T)-1 && dz == (T)((typename IntTraits<T>::U)1 << (IntTraits<T>::W - 1)))) bad = true;
      else m = dz / dx;
    }
    rec[e] = IntRec<T>{z1, m};
    if (bad) pbad[(e - xi * row) / lanes + xi * ny] = 1;
  }
}

// 1-D per query: does it fail (range test, x - x1, the interval's admissible d), and where does it land.
template <class T>
__device__ __forceinline__ bool int_query1d(const T* __restrict__ knots, uint32_t n, int mode,
                                            const IntIv* __restrict__ iv, T x, uint32_t& i, T& d) {
  i = int_lower_index(knots, n, x);
  i = NDI_CHK(i, n - 1, BC_INTERVAL);
  bool fail = mode == EX_NO && !(knots[0] <= x && x <= knots[n - 1]);
  fail |= __builtin_sub_overflow(x, knots[i], &d);
  const IntIv r = iv[i];
  fail |= (long long)d < r.lo || (long long)d > r.hi;
  return fail;
}

template <class T>
__global__ __launch_bounds__(BLOCK) void int_check1d_kernel(const T* __restrict__ q, uint64_t nq,
                                                            const T* __restrict__ knots, uint32_t n, int mode,
                                                            const IntIv* __restrict__ iv,
                                                            unsigned long long* __restrict__ first_fail) {
  for (uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; j < nq; j += (uint64_t)gridDim.x * BLOCK) {
    uint32_t i;
    T d;
    if (int_query1d(knots, n, mode, iv, q[j], i, d)) atomicMin(first_fail, (unsigned long long)j);
  }
}

// WAVE = false: element e = (query, lane) per thread; WAVE = true: one query per wavefront.  CHECK: report failing
// queries (and skip their rows); without it every query is taken to be valid (the rows before the first failure).
template <class T, bool WAVE, bool CHECK>
__global__ __launch_bounds__(BLOCK) void int_eval1d_kernel(const T* __restrict__ q, uint64_t nq,
                                                           const T* __restrict__ knots, uint32_t n, int mode,
                                                           const IntIv* __restrict__ iv,
                                                           const IntRec<T>* __restrict__ rec, uint64_t lanes,
                                                           T* __restrict__ out, uint64_t stride,
                                                           unsigned long long* __restrict__ first_fail) {
  if (WAVE) {
    const uint64_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (BLOCK / 64);
    for (uint64_t j = (uint64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); j < nq; j += waves) {
      uint32_t i;
      T d;
      const bool fail = int_query1d(knots, n, mode, iv, q[j], i, d);
      if (CHECK && fail) {
        if (lane == 0) atomicMin(first_fail, (unsigned long long)j);
        continue;
      }
      const IntRec<T>* r = rec + (uint64_t)i * lanes;
      T* o = out + j * stride;
      for (uint64_t l = lane; l < lanes; l += 64) {
        const IntRec<T> a = r[l];
        o[l] = wrap_mad(a.m, d, a.v);
      }
    }
  } else {
    const uint64_t total = nq * lanes;
    for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (uint64_t)gridDim.x * BLOCK) {
      const uint64_t j = lanes == 1 ? e : e / lanes;
      const uint64_t l = e - j * lanes;
      uint32_t i;
      T d;
      const bool fail = int_query1d(knots, n, mode, iv, q[j], i, d);
      if (CHECK && fail) {
        if (l == 0) atomicMin(first_fail, (unsigned long long)j);
        continue;
      }
      const IntRec<T> a = rec[(uint64_t)i * lanes + l];
      out[j * stride + l] = wrap_mad(a.m, d, a.v);
    }
  }
}

// 2-D per query: the range tests, both searches, x - x1, y - y1 and the marks of the two points and the y interval.
template <class T>
struct IntQuery2 {
  uint32_t xi, yi;
  T dx, dy;
  bool fail;
};
template <class T>
__device__ __forceinline__ IntQuery2<T> int_query2d(const T* __restrict__ kx, uint32_t nx, const T* __restrict__ ky,
                                                    uint32_t ny, int mode, const uint8_t* __restrict__ pbad,
                                                    const IntYIv<T>* __restrict__ yiv, T x, T y) {
  IntQuery2<T> Q;
  Q.xi = NDI_CHK(int_lower_index(kx, nx, x), nx - 1, BC_CELL_X);
  Q.yi = NDI_CHK(int_lower_index(ky, ny, y), ny - 1, BC_CELL_Y);
  bool f = mode == EX_NO && !(kx[0] <= x && x <= kx[nx - 1] && ky[0] <= y && y <= ky[ny - 1]);
  f |= __builtin_sub_overflow(x, kx[Q.xi], &Q.dx);
  f |= __builtin_sub_overflow(y, ky[Q.yi], &Q.dy);
  const uint64_t p = (uint64_t)Q.xi * ny + Q.yi;
  f |= (pbad[p] | pbad[p + 1]) != 0;
  f |= yiv[Q.yi].bad != 0;
  Q.fail = f;
  return Q;
}

// One lane of Bilinear::interp_into (bilinear.rs:88-97): z1, z2 along x from the point records, then along y.
template <class T>
__device__ __forceinline__ bool int_bilinear_lane(const IntRec<T>& a, const IntRec<T>& b, T dx, T dy,
                                                  const IntMagic<T>& mg, T& res) {
  T p1, z1, p2, z2, dz, p3;
  bool f = __builtin_mul_overflow(a.m, dx, &p1);
  f |= __builtin_add_overflow(p1, a.v, &z1);
  f |= __builtin_mul_overflow(b.m, dx, &p2);
  f |= __builtin_add_overflow(p2, b.v, &z2);
  f |= __builtin_sub_overflow(z2, z1, &dz);
  const T m = int_div_magic<T>(dz, mg);
  f |= __builtin_mul_overflow(m, dy, &p3);
  f |= __builtin_add_overflow(p3, z1, &res);
  return f;
}

template <class T, bool WAVE, bool CHECK, bool WRITE>
__global__ __launch_bounds__(BLOCK) void int_eval2d_kernel(const T* __restrict__ qx, const T* __restrict__ qy,
                                                           uint64_t nq, const T* __restrict__ kx, uint32_t nx,
                                                           const T* __restrict__ ky, uint32_t ny, int mode,
                                                           const uint8_t* __restrict__ pbad,
                                                           const IntYIv<T>* __restrict__ yiv,
                                                           const IntRec<T>* __restrict__ rec, uint64_t lanes,
                                                           T* __restrict__ out, uint64_t stride,
                                                           unsigned long long* __restrict__ first_fail) {
  if (WAVE) {
    const uint64_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (BLOCK / 64);
    for (uint64_t j = (uint64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); j < nq; j += waves) {
      const IntQuery2<T> Q = int_query2d(kx, nx, ky, ny, mode, pbad, yiv, qx[j], qy[j]);
      if (CHECK && Q.fail) {
        if (lane == 0) atomicMin(first_fail, (unsigned long long)j);
        continue;
      }
      const IntMagic<T> mg = yiv[Q.yi].mg;
      const IntRec<T>* r0 = rec + ((uint64_t)Q.xi * ny + Q.yi) * lanes;   // (xi, yi) then (xi, yi + 1): one run
      const IntRec<T>* r1 = r0 + lanes;
      T* o = out + j * stride;
      bool f = false;
      for (uint64_t l = lane; l < lanes; l += 64) {
        T res;
        f |= int_bilinear_lane(r0[l], r1[l], Q.dx, Q.dy, mg, res);
        if (WRITE) o[l] = res;
      }
      if (CHECK && f) atomicMin(first_fail, (unsigned long long)j);
    }
  } else {
    const uint64_t total = nq * lanes;
    for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (uint64_t)gridDim.x * BLOCK) {
      const uint64_t j = lanes == 1 ? e : e / lanes;
      const uint64_t l = e - j * lanes;
      const IntQuery2<T> Q = int_query2d(kx, nx, ky, ny, mode, pbad, yiv, qx[j], qy[j]);
      if (CHECK && Q.fail) {
        if (l == 0) atomicMin(first_fail, (unsigned long long)j);
        continue;
      }
      const IntRec<T>* r0 = rec + ((uint64_t)Q.xi * ny + Q.yi) * lanes;
      T res;
      const bool f = int_bilinear_lane(r0[l], r0[l + lanes], Q.dx, Q.dy, yiv[Q.yi].mg, res);
      if (WRITE) out[j * stride + l] = res;
      if (CHECK && f) atomicMin(first_fail, (unsigned long long)j);
    }
  }
}

}  // namespace ndi

namespace ndi {
// ndi_locator / ndi_get_lower_index_batch on integer knots (no NaN; the search is fully determined).
template <class T>
__global__ __launch_bounds__(BLOCK) void int_locate_kernel(const T* __restrict__ q, uint64_t nq,
                                                           const T* __restrict__ knots, uint32_t n,
                                                           int64_t* __restrict__ out) {
  for (uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; j < nq; j += (uint64_t)gridDim.x * BLOCK)
    out[j] = (int64_t)int_lower_index(knots, n, q[j]);
}
}  // namespace ndi
