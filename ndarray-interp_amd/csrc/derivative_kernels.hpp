// csrc/derivative_kernels.hpp -- derivative handles of the cubic evaluation class (CubicSpline, Pchip, Akima, CubicHermite).
//
// The evaluation kernels compute  (1-t) y_l + t y_r + t (1-t) (a (1-t) + b t)  for ANY tables {y, a, b}.  The derivative of
// a piecewise cubic is a piecewise quadratic, and a quadratic p is exactly (1-t) p0 + t p1 + t (1-t) c with c = -p''/2
// (a == b == c).  So a derivative is a NEW HANDLE whose three tables come from the source's three tables in one pass, and
// every evaluation kernel, the ring, shards, clones and every AUTO rule serve it unchanged.
//
//   derivative_build_kernel<T, VN>   one thread per table entry (interval i, one lane or one 16-byte vector of lanes);
//                                    consecutive threads on consecutive lanes, and on consecutive knots for scalar data
//
// Numerical contract (include/ndinterp.h, ndi_interp1d_derivative): every line below is one IEEE operation in T, in the
// stated order, nothing fused (-ffp-contract=off, correctly rounded division), so the tables are bit-identical to a numpy
// restatement in the same order (tests/derivative_ref.py).  Compulsory traffic: 4 rows in (y, y shifted by one knot comes
// from L2: it is the neighbouring thread's own row; a, b), 3 rows out = 7 n L sizeof(T); two divisions per entry.
#pragma once

namespace ndi {

template <class T>
struct DerivArgs {
  const T* y;   // source tables: [n][lanes], [n-1][lanes], [n-1][lanes]
  const T* a;
  const T* b;
  const T* x;   // [n] knots (the source pyramid's level 0)
  T* Y;         // [n][lanes]    the derivative at the knots (an interior knot: of the interval to its right)
  T* A;         // [n-1][lanes]  A == B == 3 (b - a) / dx
  T* B;
  uint64_t n, lanes;
};

// One table entry: interval i, lanes [lv * VN, lv * VN + VN).
// In-place use is relied on: the Bicubic axis passes (bicubic_host.hpp) run this with A == a and B == b.  That holds because
// y, a and b of the entry are loaded into registers before anything is stored and an entry is read and written by one
// thread only -- keep the loads ahead of the stores, and do not mark the DerivArgs pointers __restrict__.
template <class T, int VN>
__device__ __forceinline__ void derivative_entry(const DerivArgs<T>& D, uint64_t i, uint64_t lv) {
  using V = typename VecT<T, VN>::type;
  const uint64_t L = D.lanes;
  const uint64_t off = i * L + lv * VN;
  const V yl = *reinterpret_cast<const V*>(D.y + off);
  const V yr = *reinterpret_cast<const V*>(D.y + off + L);
  const V a = *reinterpret_cast<const V*>(D.a + off);
  const V b = *reinterpret_cast<const V*>(D.b + off);
  const T dx = const_load(D.x, i + 1) - const_load(D.x, i);
  const V dy = yr - yl;
  *reinterpret_cast<V*>(D.Y + off) = (dy + a) / dx;
  const V c = (T(3) * (b - a)) / dx;
  *reinterpret_cast<V*>(D.A + off) = c;
  *reinterpret_cast<V*>(D.B + off) = c;
  if (i + 2 == D.n) *reinterpret_cast<V*>(D.Y + off + L) = (dy - b) / dx;   // the last knot: the right end of interval n-2
}

template <class T, int VN>
__global__ __launch_bounds__(BLOCK) void derivative_build_kernel(DerivArgs<T> D) {
  const uint64_t LV = D.lanes / VN, total = (D.n - 1) * LV;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += step) {
    uint64_t i, lv;
    if (LV == 1) {                       // scalar data: consecutive threads on consecutive knots
      i = e;
      lv = 0;
    } else if (total <= 0xffffffffull) {   // (a 32-bit division where it serves: uniform branch)
      const uint32_t q = (uint32_t)e / (uint32_t)LV;
      i = q;
      lv = (uint32_t)e - q * (uint32_t)LV;
    } else {
      i = e / LV;
      lv = e - i * LV;
    }
    derivative_entry<T, VN>(D, NDI_CHK(i, D.n - 1, BC_INTERVAL), lv);
  }
}

}  // namespace ndi
