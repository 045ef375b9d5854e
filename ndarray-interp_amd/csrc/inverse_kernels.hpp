// csrc/inverse_kernels.hpp -- inverse handles of the 1-D interpolants (ndi_interp1d_inverse): solve f_l(x) = v on the device.
//
// An inverse handle's queries are VALUES v and its rows are abscissae.  The node table N[n][lanes] is the source's data
// table y (Linear and the cubic class) or the prefix table P (antiderivative sources); every lane of it is monotone, which
// inverse_check_kernel establishes once at creation.  Evaluation is one kernel: a binary search over the node values of
// the lane, then a bracketed Newton iteration on the interval's polynomial in t (Linear: the closed form).
//
// Numerical contract (include/ndinterp.h, ndi_interp1d_inverse): every line one IEEE operation in T, in the stated order,
// nothing fused (-ffp-contract=off, correctly rounded division); tests/inverse_ref.py restates it in numpy.
//   search   lo = 0, hi = n-1;  while hi - lo > 1:  mid = (lo + hi) >> 1
//                if (rising ? c[mid] <= v : c[mid] >= v) lo = mid else hi = mid
//            i = lo;  nl = c[i], nr = c[i+1];  xl = x[i], xr = x[i+1];  dx = xr - xl
//   start    if v == nl:  t = 0  -> finish
//            t = (v - nl) / (nr - nl)                   Linear sources: -> finish
//   solve    tl = 0, th = 1, dprev = 1;   repeat at most K times:
//                f = p(t) - v;            if f == 0: stop
//                if (rising ? f < 0 : f > 0) tl = t else th = t
//                d = p'(t);  s = f / d;  tn = t - s
//                if !(tn > tl && tn < th) or !(|s + s| <= |dprev|):  tn = tl + 0.5 * (th - tl)
//                step = tn - t;  dprev = step;  t = tn
//                if |step| <= eps_T: stop
//   finish   w = xl + t * dx;  x = (t == 1) ? xr : (w < xr ? w : xr)
//
// Mapping: one thread per output element, the flat index with lanes fastest: stores coalesce, v[j] is a broadcast, and the
// column reads c[mid * lanes + l] of neighbouring lanes coalesce while their searches agree.  The solve loop is per thread;
// a wavefront runs until its slowest lane stops.  (A form with one 16-byte group of lanes per thread, its components solved
// one after the other and stored together, was measured and dropped: equal at f64, up to 1.6 x slower at f32 -- DESIGN.md
// 4.18.)
#pragma once

namespace ndi {

enum InverseClass : int {
  IC_LINEAR = 0,        // N = y, closed form
  IC_CUBIC = 1,         // N = y, tables {y, a, b}
  IC_ANTI_CUBIC = 2,    // N = P, the quartic of antiderivative_kernels.hpp
  IC_ANTI_LINEAR = 3,   // N = P, its quadratic
};

template <class T>
struct InverseLimits;
template <>
struct InverseLimits<double> {
  static constexpr int K = 128;
  static constexpr double eps() { return 0x1p-52; }
};
template <>
struct InverseLimits<float> {
  static constexpr int K = 64;
  static constexpr float eps() { return 0x1p-23f; }
};

// ---- creation: is every lane of N monotone? -----------------------------------------------------------------------------
// flags[l] collects, over all knots of lane l:  1 = a rise (N[i+1] > N[i]), 2 = a fall, 4 = a NaN.  A lane is refused when it
// has both 1 and 2, or 4.  One thread walks INV_CHECK_RUN consecutive knots of one lane (consecutive threads on consecutive
// lanes: coalesced rows) and publishes its bits with at most one atomicOr, skipped when the word already has them (the
// plain read is only a filter: the OR is idempotent).  n x 1 tables are therefore n / INV_CHECK_RUN threads, not one loop.
constexpr uint32_t INV_CHECK_RUN = 64;

template <class T>
__global__ __launch_bounds__(BLOCK) void inverse_check_kernel(const T* N, uint64_t n, uint64_t lanes, unsigned int* flags) {
  const uint64_t runs = (n + INV_CHECK_RUN - 1) / INV_CHECK_RUN, total = runs * lanes;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += step) {
    const uint64_t r = e / lanes, l = e - r * lanes;
    const uint64_t i0 = r * INV_CHECK_RUN;
    const uint64_t i1 = (n - i0 < INV_CHECK_RUN + 1) ? n : i0 + INV_CHECK_RUN + 1;   // one past the last knot read: the
    unsigned int bits = 0;                                                          // run's pairs reach into the next run
    T prev = N[NDI_CHK(i0, n, BC_INTERVAL) * lanes + l];
    if (!(prev == prev)) bits |= 4u;
    for (uint64_t i = i0 + 1; i < i1; ++i) {
      const T cur = N[NDI_CHK(i, n, BC_INTERVAL) * lanes + l];
      if (cur > prev) bits |= 1u;
      if (cur < prev) bits |= 2u;
      if (!(cur == cur)) bits |= 4u;
      prev = cur;
    }
    if (bits && (__atomic_load_n(&flags[l], __ATOMIC_RELAXED) & bits) != bits) atomicOr(&flags[l], bits);
  }
}

// ---- evaluation -------------------------------------------------------------------------------------------------------
template <class T>
struct InverseEvalArgs {
  const T* knots;   // [n]
  const T* N;       // [n][lanes]: y (IC_LINEAR, IC_CUBIC) or P (IC_ANTI_*)
  const T* y;       // [n][lanes] (IC_ANTI_*: the source's data; otherwise == N)
  const T* a;       // [n-1][lanes] (IC_CUBIC, IC_ANTI_CUBIC)
  const T* b;
  const T* q;       // [nq] values
  T* out;           // [nq][out_stride] abscissae
  uint64_t n, lanes, out_stride, nq;
  const StatusBlock* status;   // first_fail[0]: the range pre-pass's verdict on q (rows at / after it are not written)
};

// The interval's polynomial in t as the forward evaluation of the class forms it, and its derivative in t.
template <class T, int CLASS>
struct InversePoly {
  T yl, yr, a, b, p0, dx;   // the operands
  T c1, c2, c3;             // IC_ANTI_*: as stated for ndi_interp1d_antiderivative
  T d0, e2, g;              // IC_CUBIC: dy + a, 2 (b - 2a), 3 (b - a)
  __device__ __forceinline__ void prepare() {
    if constexpr (CLASS == IC_CUBIC) {
      const T dy = yr - yl;
      d0 = dy + a;
      const T e = b - (a + a);
      e2 = e + e;
      g = T(3) * (b - a);
    } else if constexpr (CLASS == IC_ANTI_CUBIC) {
      const T dy = yr - yl;
      c1 = (dy + a) * T(0.5);
      c2 = (b - (a + a)) / T(3);
      c3 = (b - a) * T(0.25);
    } else if constexpr (CLASS == IC_ANTI_LINEAR) {
      c1 = (yr - yl) * T(0.5);
    }
  }
  __device__ __forceinline__ T value(T t) const {
    if constexpr (CLASS == IC_CUBIC) {
      const T u = T(1) - t;
      return (u * yl + t * yr) + (t * u) * (a * u + b * t);
    } else if constexpr (CLASS == IC_ANTI_CUBIC) {
      return p0 + dx * (t * (yl + t * (c1 + t * (c2 - t * c3))));
    } else {
      return p0 + dx * (t * (yl + t * c1));
    }
  }
  __device__ __forceinline__ T slope(T t) const {
    if constexpr (CLASS == IC_CUBIC) {
      return d0 + t * (e2 - g * t);
    } else if constexpr (CLASS == IC_ANTI_CUBIC) {
      return dx * (yl + t * ((c1 + c1) + t * (T(3) * c2 - (T(4) * c3) * t)));
    } else {
      return dx * (yl + t * (c1 + c1));
    }
  }
};

__device__ __forceinline__ float inverse_abs(float v) { return __builtin_fabsf(v); }
__device__ __forceinline__ double inverse_abs(double v) { return __builtin_fabs(v); }

// x with f_l(x) = v: the whole contract for one output element.
template <class T, int CLASS>
__device__ __forceinline__ T inverse_element(const InverseEvalArgs<T>& A, T v, uint64_t l) {
  const uint64_t L = A.lanes, n = A.n;
  const T* c = A.N + l;
  const bool rising = c[(n - 1) * L] >= c[0];
  uint64_t lo = 0, hi = n - 1;
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    const T cm = c[NDI_CHK(mid, n, BC_INTERVAL) * L];
    if (rising ? cm <= v : cm >= v) lo = mid;
    else hi = mid;
  }
  const uint64_t i = NDI_CHK(lo, n - 1, BC_INTERVAL);
  const T nl = c[i * L], nr = c[(i + 1) * L];
  const T xl = const_load(A.knots, i), xr = const_load(A.knots, i + 1);
  const T dx = xr - xl;
  T t = T(0);
  if (!(v == nl)) {
    t = (v - nl) / (nr - nl);
    if constexpr (CLASS != IC_LINEAR) {
      InversePoly<T, CLASS> p;
      p.dx = dx;
      p.p0 = nl;
      if constexpr (CLASS == IC_CUBIC) {
        p.yl = nl;
        p.yr = nr;
      } else {
        p.yl = A.y[i * L + l];
        p.yr = A.y[(i + 1) * L + l];
      }
      if constexpr (CLASS != IC_ANTI_LINEAR) {
        p.a = A.a[i * L + l];
        p.b = A.b[i * L + l];
      }
      p.prepare();
      T tl = T(0), th = T(1), dprev = T(1);
      for (int k = 0; k < InverseLimits<T>::K; ++k) {
        const T f = p.value(t) - v;
        if (f == T(0)) break;
        if (rising ? f < T(0) : f > T(0)) tl = t;
        else th = t;
        const T d = p.slope(t);
        const T s = f / d;
        T tn = t - s;
        if (!(tn > tl && tn < th) || !(inverse_abs(s + s) <= inverse_abs(dprev))) tn = tl + T(0.5) * (th - tl);
        const T step = tn - t;
        dprev = step;
        t = tn;
        if (inverse_abs(step) <= InverseLimits<T>::eps()) break;
      }
    }
  }
  const T w = xl + t * dx;
  return (t == T(1)) ? xr : (w < xr ? w : xr);
}

template <class T, int CLASS>
__global__ __launch_bounds__(BLOCK) void inverse_eval_kernel(InverseEvalArgs<T> A) {
  const uint64_t L = A.lanes;
  unsigned long long limit = A.status->first_fail[0];
  if (limit > A.nq) limit = A.nq;
  const uint64_t total = limit * L;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += step) {
    uint64_t qi, l;
    if (total <= 0xFFFFFFFFull) {   // 32-bit division where the batch allows (the uniform branch costs nothing)
      const uint32_t q32 = (uint32_t)e / (uint32_t)L;
      qi = q32;
      l = (uint32_t)e - q32 * (uint32_t)L;
    } else {
      qi = e / L;
      l = e - qi * L;
    }
    const T v = A.q[NDI_CHK(qi, A.nq, BC_QUERY)];
    A.out[qi * A.out_stride + l] = inverse_element<T, CLASS>(A, v, l);
  }
}

}  // namespace ndi
