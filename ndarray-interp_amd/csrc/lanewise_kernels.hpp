// csrc/lanewise_kernels.hpp -- lane-wise evaluation of the 1-D handles (ndi_interp1d_eval_lanewise): a query per lane,
//     out[j][l] = f_l(q[j][l]).
//
// Value rule (include/ndinterp.h): out[j][l] is, bit for bit, element l of the row ndi_interp1d_eval writes for the single
// query q[j][l].  The kernels get it by construction: the search is locate_index / locate_kernel, the wrap rem_euclid_t,
// the point RowCoef / row_point (antiderivatives: antideriv_point, inverses: inverse_element), nothing re-associated.
//
// Mapping, all kernels: one thread per output ELEMENT, the flat index e = j * lanes + l with lanes fastest, so a wavefront
// takes 64 consecutive elements and its query loads and stores coalesce (a row pitch above lanes only adds the gap between
// rows).  The split of e into (row, lane) is ONE 64-bit division per thread, before the loop; the grid stride is handed in
// as (step_rows, step_lanes) = (step / lanes, step % lanes) and every trip advances (j, l) by it with one carry -- no
// division in the loop whatever the strides (the lane is needed in every case: the tables are [n][lanes]).
//
//   eval_lanewise_kernel     Linear / the cubic class, the search fused in (the sibling of eval_small_kernel): every lane of
//                            the wavefront carries its own query through the wave-cooperative locate_index, or through
//                            the axis' bucket index where locate_kernel would use it; the knot pyramid (and the index)
//                            is staged in LDS when it fits (STAGE), else read from global memory
//   lanewise_point_kernel    the element kernel of the two-kernel form: idx[] / t[] from locate_kernel over the flat
//                            queries; Linear, the cubic class and both antiderivative classes
//   inverse_lanewise_kernel  inverse handles: inverse_element(A, q[j][l], l)
//   lanewise_check_kernel    the pre-pass: the lowest failing flat element index (shared limits and the mode's rule, or
//                            per-lane limit arrays)
//   lanewise_records_kernel  the element-record copy R[i][l] = {y[i][l], y[i+1][l], a[i][l], b[i][l]} (Linear: the first
//                            two): with a query per lane neighbouring threads usually sit in different intervals and the
//                            plain tables cost four scattered element reads per output; a record is ONE aligned 16- or
//                            32-byte load (Linear: 8 / 16).  Values are copied, never recomputed.  (Letting a wavefront
//                            whose lanes share one interval read the plain rows instead was measured and dropped: up to
//                            1.5 x slower on short rows, no gain on long ones -- DESIGN.md 4.19.)
#pragma once

namespace ndi {

// The position of a thread's element and the stride that advances it.
struct LanewiseGeom {
  uint64_t lanes, rows;            // rows: nq
  uint64_t q_stride, out_stride;   // row pitches in elements (>= lanes)
  uint64_t step_rows, step_lanes;  // (gridDim.x * BLOCK) / lanes and % lanes
};

struct LanewisePos {
  uint64_t j, l;
  __device__ __forceinline__ void start(const LanewiseGeom& G, uint64_t e) {
    j = e / G.lanes;
    l = e - j * G.lanes;
  }
  __device__ __forceinline__ void advance(const LanewiseGeom& G) {
    j += G.step_rows;
    l += G.step_lanes;
    if (l >= G.lanes) {
      l -= G.lanes;
      ++j;
    }
  }
};

// Rows that may be written: all of them when the kernel tests the queries itself, else the rows before the row of the
// first failing element (first_fail: the pre-pass's, or locate_kernel's).
__device__ __forceinline__ uint64_t lanewise_rows(const LanewiseGeom& G, const unsigned long long* first_fail, int check) {
  if (check) return G.rows;
  const unsigned long long f = *first_fail;
  if (f == NO_FAIL) return G.rows;
  const uint64_t r = f / G.lanes;
  return r < G.rows ? r : G.rows;
}

// ---- element records ----------------------------------------------------------------------------------------------------
template <class T, int PARTS>
struct alignas(sizeof(T) * PARTS) LanewiseRecord {
  T v[PARTS];
};

template <class T, int PARTS>
__global__ __launch_bounds__(BLOCK) void lanewise_records_kernel(const T* data, const T* ca, const T* cb,
                                                                 LanewiseRecord<T, PARTS>* out, uint64_t n, uint64_t lanes) {
  const uint64_t total = (n - 1) * lanes;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (uint64_t)gridDim.x * BLOCK) {
    LanewiseRecord<T, PARTS> r;
    r.v[0] = data[e];
    r.v[1] = data[e + lanes];
    if constexpr (PARTS == 4) {
      r.v[2] = ca[e];
      r.v[3] = cb[e];
    }
    out[e] = r;
  }
}

// ---- the pre-pass -------------------------------------------------------------------------------------------------------
// lo == nullptr: the shared limits [x0, xn] with the mode's rule, exactly range_check_kernel's test.  Otherwise the
// per-lane limits of an inverse handle: v outside [lo[l], hi[l]] (inclusive; a NaN compares false) fails.
template <class T>
__global__ __launch_bounds__(BLOCK) void lanewise_check_kernel(const T* q, LanewiseGeom G, T x0, T xn, int mode, const T* lo,
                                                               const T* hi, unsigned long long* first_fail) {
  const uint64_t total = G.rows * G.lanes;
  uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= total) return;
  LanewisePos p;
  p.start(G, e);
  for (; e < total; e += (uint64_t)gridDim.x * BLOCK, p.advance(G)) {
    const uint64_t j = NDI_CHK(p.j, G.rows, BC_QUERY), l = NDI_CHK(p.l, G.lanes, BC_LANE);
    const T x = q[j * G.q_stride + l];
    bool bad;
    if (lo) {
      bad = !((lo[l] <= x) && (x <= hi[l]));
    } else {
      const bool inr = (x0 <= x) && (x <= xn);
      T xs = x;
      if (mode == EX_PERIODIC && !inr) xs = rem_euclid_t(x - x0, xn - x0) + x0;   // +-inf wraps to NaN, as in locate_slice
      bad = (mode == EX_NO) ? !inr : !(xs == xs);
    }
    if (bad) atomicMin(first_fail, (unsigned long long)e);
  }
}

// ---- Linear / the cubic class, search fused in ---------------------------------------------------------------------------
template <class T>
struct LanewiseArgs {
  Pyramid<T> pyr;
  BucketIndex<T> bx;      // bucket index staged behind the pyramid when bx.lut != nullptr (STAGE), as locate_kernel has it
  BucketIndex32<T> bx32;  // bucket index read from global memory (axes that are not staged)
  const T* data;   // [n][lanes]
  const T* ca;     // [n-1][lanes] (cubic class)
  const T* cb;
  const void* rec; // element records [n-1][lanes] (REC), else unused
  const T* q;      // [rows][q_stride]
  T* out;          // [rows][out_stride]
  LanewiseGeom G;
  int mode;        // ExtrapMode
  int check;       // 1: the kernel tests the queries itself and publishes the lowest failing element; 0: first_fail holds it
  unsigned long long* first_fail;
};

template <class T, int STRAT, bool STAGE, bool REC>
__global__ __launch_bounds__(BLOCK) void eval_lanewise_kernel(LanewiseArgs<T> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  using PTR = typename std::conditional<STAGE, lds_ptr<T>, const T*>::type;
  constexpr int PARTS = STRAT == ST_CUBIC ? 4 : 2;
  const uint32_t tid = threadIdx.x;
  const uint32_t n = A.pyr.n, n1 = A.pyr.n1;
  PyramidT<T, PTR> P;
  lds_u16 lut = nullptr;
  if constexpr (STAGE) {
    T* s0 = reinterpret_cast<T*>(smem_raw);
    const uint32_t total = n + n1;   // the levels are one allocation
    for (uint32_t i = tid; i < total; i += BLOCK) s0[i] = A.pyr.lv0[i];
    if (A.bx.lut) {   // [pyramid | lut]; the lut is copied as 32-bit words (m + 1 entries, padded)
      const size_t lut_off = ((size_t)total * sizeof(T) + 15u) & ~(size_t)15u;
      uint32_t* sl = reinterpret_cast<uint32_t*>(smem_raw + lut_off);
      const uint32_t words = (A.bx.m + 2u) / 2u;
      const uint32_t* src = reinterpret_cast<const uint32_t*>(A.bx.lut);
      for (uint32_t i = tid; i < words; i += BLOCK) sl[i] = src[i];
      lut = (lds_u16)(smem_raw + lut_off);
    }
    __syncthreads();
    P.lv0 = (lds_ptr<T>)(smem_raw);
    P.lv1 = P.lv0 + n;
  } else {
    P.lv0 = A.pyr.lv0;
    P.lv1 = A.pyr.lv1;
  }
  P.n = n; P.n1 = n1; P.levels = A.pyr.levels; P.guess = A.pyr.guess; P.block = A.pyr.block;
  const T k0 = P.lv0[0], kn = P.lv0[n - 1];
  const uint32_t lane = tid & 63u;
  const LanewiseGeom G = A.G;
  const uint64_t L = G.lanes;
  const uint64_t total = lanewise_rows(G, A.first_fail, A.check) * L;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  uint64_t base = (uint64_t)blockIdx.x * BLOCK + (tid & ~63u);   // wave-uniform: all 64 lanes run the same trips
  if (base >= total) return;                                      // (no barrier follows)
  LanewisePos p;
  p.start(G, base + lane);
  for (; base < total; base += step, p.advance(G)) {
    const uint64_t e = base + lane;
    const bool active = e < total;
    const uint64_t j = active ? NDI_CHK(p.j, G.rows, BC_QUERY) : 0, l = active ? NDI_CHK(p.l, L, BC_LANE) : 0;
    const T x = active ? A.q[j * G.q_stride + l] : k0;   // inactive lanes take part with the first knot
    const bool inr = (k0 <= x) && (x <= kn);
    T xs = x;
    if (A.mode == EX_PERIODIC && !inr) xs = rem_euclid_t(x - k0, kn - k0) + k0;
    // unique i with k[i] <= x < k[i+1], clamped to [0, n-2], by the search locate_kernel would take on this axis
    uint32_t i;
    if constexpr (STAGE) {
      i = lut ? locate_index_lut<T>(P, lut, A.bx.m, A.bx.scale, k0, kn, xs) : locate_index<T, PTR>(P, k0, kn, xs, lane);
    } else if (A.bx32.lut) {
      const uint32_t ub = lut32_count_le<T>(P.lv0, n, A.bx32.lut, A.bx32.m, A.bx32.scale, k0, kn, xs);
      i = (ub == 0) ? 0u : ub - 1u;
      if (i > n - 2u) i = n - 2u;
    } else {
      i = locate_index<T, PTR>(P, k0, kn, xs, lane);   // all 64 lanes take part
    }
    if (!active) continue;
    const bool bad = (A.mode == EX_NO) ? !inr : !(xs == xs);
    if (bad) {
      if (A.check) atomicMin(A.first_fail, (unsigned long long)e);
      continue;
    }
    i = NDI_CHK(i, n - 1u, BC_INTERVAL);
    const T xl = P.lv0[i], xr = P.lv0[i + 1];
    RowCoef<T, STRAT> c;
    if (STRAT == ST_CUBIC) {
      const T t = (xs - xl) / (xr - xl);   // cubic_spline.rs:818
      const T one = T(1);
      c.c0 = one - t;
      c.c1 = t;
      c.c2 = t * (one - t);
    } else {
      c.c0 = xr - xl;
      c.c1 = x - xl;
      c.c2 = T(0);
    }
    const uint64_t at = (uint64_t)i * L + l;
    T yl, yr, a = T(0), b = T(0);
    if constexpr (REC) {
      const LanewiseRecord<T, PARTS> r = static_cast<const LanewiseRecord<T, PARTS>*>(A.rec)[at];
      yl = r.v[0];
      yr = r.v[1];
      if constexpr (STRAT == ST_CUBIC) {
        a = r.v[2];
        b = r.v[3];
      }
    } else {
      yl = A.data[at];
      yr = A.data[at + L];
      if (STRAT == ST_CUBIC) {
        a = A.ca[at];
        b = A.cb[at];
      }
    }
    A.out[j * G.out_stride + l] = row_point<T, STRAT, T>(c, yl, yr, a, b);
  }
}

// ---- the element kernel of the two-kernel form ---------------------------------------------------------------------------
enum LanewiseKind : int { LW_LINEAR = 0, LW_CUBIC = 1, LW_ANTI_LINEAR = 2, LW_ANTI_CUBIC = 3 };

template <class T>
struct LanewisePointArgs {
  const T* knots;
  const T* y;      // [n][lanes]
  const T* a;      // [n-1][lanes] (cubic classes)
  const T* b;
  const T* P;      // [n][lanes] (antiderivative classes)
  const T* q;      // [rows][q_stride]: Linear evaluates on the query itself
  const uint32_t* idx;   // [rows * lanes]: interval and t per flat element (locate_kernel)
  const T* t;
  T* out;
  LanewiseGeom G;
  const unsigned long long* first_fail;   // locate_kernel's verdict: rows at / after its row are not written
  uint32_t n_int;                         // n - 1: limit of every interval index (checked build)
};

template <class T, int KIND>
__global__ __launch_bounds__(BLOCK) void lanewise_point_kernel(LanewisePointArgs<T> A) {
  const LanewiseGeom G = A.G;
  const uint64_t L = G.lanes;
  const uint64_t total = lanewise_rows(G, A.first_fail, 0) * L;
  uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= total) return;
  LanewisePos p;
  p.start(G, e);
  for (; e < total; e += (uint64_t)gridDim.x * BLOCK, p.advance(G)) {
    const uint64_t j = NDI_CHK(p.j, G.rows, BC_QUERY), l = NDI_CHK(p.l, L, BC_LANE);
    const uint32_t i = NDI_CHK(A.idx[e], A.n_int, BC_INTERVAL);
    const uint64_t at = (uint64_t)i * L + l;
    const T yl = A.y[at], yr = A.y[at + L];
    T a = T(0), b = T(0);
    if constexpr (KIND == LW_CUBIC || KIND == LW_ANTI_CUBIC) {
      a = A.a[at];
      b = A.b[at];
    }
    T r;
    if constexpr (KIND == LW_LINEAR || KIND == LW_CUBIC) {
      constexpr int STRAT = KIND == LW_CUBIC ? ST_CUBIC : ST_LINEAR;
      const RowCoef<T, STRAT> c = row_coef<T, STRAT>(A.knots, i, STRAT == ST_LINEAR ? A.q[j * G.q_stride + l] : T(0),
                                                     STRAT == ST_CUBIC ? A.t[e] : T(0));
      r = row_point<T, STRAT, T>(c, yl, yr, a, b);
    } else {
      const T dx = A.knots[i + 1] - A.knots[i];
      r = A.P[at] + antideriv_point<KIND == LW_ANTI_LINEAR, T, T>(yl, yr, a, b, dx, A.t[e]);
    }
    A.out[j * G.out_stride + l] = r;
  }
}

// ---- inverse handles ----------------------------------------------------------------------------------------------------
template <class T>
struct LanewiseInverseArgs {
  InverseEvalArgs<T> A;   // the tables (q / out / out_stride / nq / status of it are not read)
  const T* q;             // [rows][q_stride] values
  T* out;                 // [rows][out_stride] abscissae
  const T* lo;            // [lanes]: lane l's own value range
  const T* hi;
  LanewiseGeom G;
  int check;              // as LanewiseArgs
  unsigned long long* first_fail;
};

template <class T, int CLASS>
__global__ __launch_bounds__(BLOCK) void inverse_lanewise_kernel(LanewiseInverseArgs<T> W) {
  const LanewiseGeom G = W.G;
  const uint64_t L = G.lanes;
  const uint64_t total = lanewise_rows(G, W.first_fail, W.check) * L;
  uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= total) return;
  LanewisePos p;
  p.start(G, e);
  for (; e < total; e += (uint64_t)gridDim.x * BLOCK, p.advance(G)) {
    const uint64_t j = NDI_CHK(p.j, G.rows, BC_QUERY), l = NDI_CHK(p.l, L, BC_LANE);
    const T v = W.q[j * G.q_stride + l];
    if (!((W.lo[l] <= v) && (v <= W.hi[l]))) {   // outside the lane's range, or NaN: the search has no interval for it
      if (W.check) atomicMin(W.first_fail, (unsigned long long)e);
      continue;
    }
    W.out[j * G.out_stride + l] = inverse_element<T, CLASS>(W.A, v, l);
  }
}

}  // namespace ndi
