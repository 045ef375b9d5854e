// csrc/hermite_kernels.hpp -- the local C1 cubics: Pchip, Akima and CubicHermite (caller-given derivatives), f32 / f64.
//
// CubicSplineStrategy::interp_into (cubic_spline.rs:811-828) evaluates the cubic Hermite form for ANY knot derivatives k
// once the tables  a_i = k_i h_i - dy,  b_i = dy - k_{i+1} h_i  (cubic_spline.rs:362-363) exist; the Thomas solve is one
// way to choose k.  The strategies here choose k from a few neighbouring rows, so their build is ONE pass with no
// recurrence along the knots, and every evaluation kernel of the spline serves their handles unchanged.
//
//   hermite_build_kernel<T, RULE, VN>   one thread per table entry (interval i, one lane or one 16-byte vector of lanes);
//                                       consecutive threads on consecutive lanes, and on consecutive knots for scalar data
//   ... <T, RULE, 1, true>              LANE_X: the knots are a table x[n][lanes] read per lane (lane_axes_kernels.hpp);
//                                       the stencil is the same code on h_i = x[i+1][l] - x[i][l]
//
// Numerical contract (include/ndinterp.h, ndi_strategy1d): every line below is one IEEE operation in T, in the stated
// order, nothing fused (-ffp-contract=off, correctly rounded division), so the tables are bit-identical to a numpy
// restatement in the same order (tests/hermite_ref.py).  h_i = x[i+1] - x[i], delta_i = (y[i+1] - y[i]) / h_i.
#pragma once

namespace ndi {

// How a handle of the cubic evaluation class got its knot derivatives.
enum HermiteRule : int { HR_SPLINE = 0, HR_PCHIP = 1, HR_AKIMA = 2, HR_GIVEN = 3 };

template <class T>
struct HermiteArgs {
  const T* data;   // [n][lanes]
  const T* x;      // [n] knots (the pyramid's level 0); LANE_X: [n][lanes], a column of knots per lane
  const T* dydx;   // HR_GIVEN: [n][lanes] derivatives
  T* ca;           // [n-1][lanes]
  T* cb;           // [n-1][lanes]
  T* kout;         // [n][lanes] or nullptr: the derivatives, for the evaluation forms that keep {y, k} in LDS
  uint64_t n, lanes;
};

__device__ __forceinline__ float hermite_abs(float v) { return fabsf(v); }
__device__ __forceinline__ double hermite_abs(double v) { return fabs(v); }
template <class T>
__device__ __forceinline__ int hermite_sgn(T v) { return (int)(v > T(0)) - (int)(v < T(0)); }

template <class T, int VN>
__device__ __forceinline__ T hermite_get(const typename VecT<T, VN>::type& v, int c) {
  if constexpr (VN == 1) return v;
  else return v[c];
}
template <class T, int VN>
__device__ __forceinline__ void hermite_set(typename VecT<T, VN>::type& v, int c, T s) {
  if constexpr (VN == 1) v = s;
  else v[c] = s;
}

// Pchip, interior knot i (Fritsch-Butland): hp = h_{i-1}, hc = h_i, dp = delta_{i-1}, dc = delta_i
template <class T>
__device__ __forceinline__ T pchip_interior(T hp, T hc, T dp, T dc) {
  if (dp == T(0) || dc == T(0) || ((dp > T(0)) != (dc > T(0)))) return T(0);
  const T w1 = (hc + hc) + hp;
  const T w2 = hc + (hp + hp);
  return (w1 + w2) / (w1 / dp + w2 / dc);
}

// Pchip, end knot: the three-point shape-preserving formula; (h0, m0) the end interval, (h1, m1) its neighbour
template <class T>
__device__ __forceinline__ T pchip_edge(T h0, T h1, T m0, T m1) {
  const T d = (((h0 + h0) + h1) * m0 - h0 * m1) / (h0 + h1);
  if (hermite_sgn(d) != hermite_sgn(m0)) return T(0);
  if (hermite_sgn(m0) != hermite_sgn(m1) && hermite_abs(d) > T(3) * hermite_abs(m0)) return T(3) * m0;
  return d;
}

// Akima (1970), knot i: mm2 = m_{i-2}, mm1 = m_{i-1}, m0 = m_i, mp1 = m_{i+1}.  The average is taken for s == 0 exactly
// (scipy: below a threshold relative to the largest s of the whole array).
template <class T>
__device__ __forceinline__ T akima_knot(T mm2, T mm1, T m0, T mp1) {
  const T w1 = hermite_abs(mp1 - m0);
  const T w2 = hermite_abs(mm1 - mm2);
  const T s = w1 + w2;
  if (s == T(0)) return T(0.5) * (mm1 + m0);
  return (w1 * mm1 + w2 * m0) / s;
}

// Akima's end extension for the window of interval i: m[w] = m_{i-2+w}, the data's slopes where 0 <= i-2+w <= n-2, else the
// linear extension, formed outwards.  (Shared with the 2-D node build, bicubic_local_kernels.hpp.)
template <class T>
__device__ __forceinline__ void akima_extend(T (&m)[5], uint64_t i, uint64_t n) {
  if (i + 1 < 2) m[1] = (m[2] + m[2]) - m[3];          // m_{-1}
  if (i + 0 < 2) m[0] = (m[1] + m[1]) - m[2];          // m_{-1} (i == 1) or m_{-2} (i == 0)
  if (i + 3 > n) m[3] = (m[2] + m[2]) - m[1];          // m_{n-1}
  if (i + 4 > n) m[4] = (m[3] + m[3]) - m[2];          // m_{n-1} (i == n-3) or m_n (i == n-2)
}

// One table entry: interval i, lanes [lv * VN, lv * VN + VN).  Reads rows i - HALO .. i + 1 + HALO where they exist
// (the neighbouring rows are other threads' own rows: they come from L2), forms k_i and k_{i+1}, writes a_i, b_i.
template <class T, int RULE, int VN, bool LANE_X = false>
__device__ __forceinline__ void hermite_entry(const HermiteArgs<T>& A, uint64_t i, uint64_t lv) {
  using V = typename VecT<T, VN>::type;
  static_assert(!LANE_X || VN == 1, "a knot column per lane: one lane per thread");
  const uint64_t n = A.n, L = A.lanes;
  const uint64_t off = i * L + lv * VN;
  constexpr int HALO = RULE == HR_AKIMA ? 2 : (RULE == HR_PCHIP ? 1 : 0);
  constexpr int ROWS = 2 + 2 * HALO;
  V y[ROWS];
  T xs[ROWS];
#pragma unroll
  for (int w = 0; w < ROWS; ++w) {
    const bool ok = i + w >= (uint64_t)HALO && i + w - HALO < n;
    y[w] = V(0);
    xs[w] = T(0);
    if (ok) {
      y[w] = *reinterpret_cast<const V*>(A.data + (off + (uint64_t)w * L - (uint64_t)HALO * L));
      if constexpr (LANE_X) xs[w] = A.x[off + (uint64_t)w * L - (uint64_t)HALO * L];
      else xs[w] = const_load(A.x, i + w - HALO);
    }
  }
  const T hi = xs[HALO + 1] - xs[HALO];
  const V dy = y[HALO + 1] - y[HALO];
  V k0, k1;
  if constexpr (RULE == HR_GIVEN) {
    k0 = *reinterpret_cast<const V*>(A.dydx + off);
    k1 = *reinterpret_cast<const V*>(A.dydx + off + L);
  } else {
    constexpr int ND = ROWS - 1;       // slopes delta_{i-HALO} .. delta_{i+HALO}; [HALO] is this interval's
    T h[ND];
    V dl[ND];
#pragma unroll
    for (int w = 0; w < ND; ++w) {
      h[w] = xs[w + 1] - xs[w];
      dl[w] = (y[w + 1] - y[w]) / h[w];   // (rows that do not exist give 0 / 0 here; never used below)
    }
#pragma unroll
    for (int c = 0; c < VN; ++c) {
      T r0, r1;
      if constexpr (RULE == HR_PCHIP) {
        const T d0 = hermite_get<T, VN>(dl[0], c), d1 = hermite_get<T, VN>(dl[1], c), d2 = hermite_get<T, VN>(dl[2], c);
        if (n == 2) {
          r0 = d1;
          r1 = d1;
        } else {
          r0 = i == 0 ? pchip_edge(h[1], h[2], d1, d2) : pchip_interior(h[0], h[1], d0, d1);
          r1 = i + 2 == n ? pchip_edge(h[1], h[0], d1, d0) : pchip_interior(h[1], h[2], d1, d2);
        }
      } else {
        T m[5];
#pragma unroll
        for (int w = 0; w < 5; ++w) m[w] = hermite_get<T, VN>(dl[w], c);
        akima_extend(m, i, n);
        r0 = akima_knot(m[0], m[1], m[2], m[3]);
        r1 = akima_knot(m[1], m[2], m[3], m[4]);
      }
      hermite_set<T, VN>(k0, c, r0);
      hermite_set<T, VN>(k1, c, r1);
    }
  }
  *reinterpret_cast<V*>(A.ca + off) = k0 * hi - dy;
  *reinterpret_cast<V*>(A.cb + off) = dy - k1 * hi;
  if (A.kout) {
    *reinterpret_cast<V*>(A.kout + off) = k0;
    if (i + 2 == n) *reinterpret_cast<V*>(A.kout + off + L) = k1;
  }
}

template <class T, int RULE, int VN, bool LANE_X = false>
__global__ __launch_bounds__(BLOCK) void hermite_build_kernel(HermiteArgs<T> A) {
  const uint64_t LV = A.lanes / VN, total = (A.n - 1) * LV;
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
    hermite_entry<T, RULE, VN, LANE_X>(A, NDI_CHK(i, A.n - 1, BC_INTERVAL), lv);
  }
}

}  // namespace ndi
