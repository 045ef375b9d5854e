// csrc/lane_axes_kernels.hpp -- 1-D handles with an x axis PER LANE (ndi_interp1d_create_lane_axes): the knots are a table
// x[n][lanes] laid out like the data, column l holds the knots of lane l, and lane l is the interpolant of
// (x[:, l], data[:, l]) alone.
//
// Value rules (include/ndinterp.h, ndi_interp1d_create_lane_axes):
//   build       column l of the a / b tables is, bit for bit, what the shared-axis handle built from (x[:, l], data[:, l])
//               with NDI_BUILD_REFERENCE_ORDER holds.  Every line below is one IEEE operation in T, nothing fused
//               (-ffp-contract=off, correctly rounded division).
//   evaluation  out[j][l] is, bit for bit and zero signs included, element 0 of the row ndi_interp1d_eval writes for that
//               query on the single-column handle of lane l: the search below finds the interval locate_kernel finds
//               (the unique i with x[i] <= q < x[i+1], clamped to [0, n-2]) and the point is row_point on the operands
//               eval_lanewise_kernel forms -- nothing restated.
//
//   lane_axes_check_kernel    creation, device-resident axes: is every column strictly rising with no NaN?  One flag word
//                             per lane, at most one atomic per run of knots (inverse_check_kernel's shape)
//   lane_axes_spline_kernel   the CubicSpline build: one thread per lane walks the Thomas recurrence over n, the diagonals
//                             low / mid / up, the factor w and the eliminated diagonal formed per lane from the lane's own
//                             knots in the operation order of the host plan (host_logic.hpp, make_spline_plan; the
//                             reference: cubic_spline.rs:409-721, a / b :350-365).  Consecutive threads take consecutive
//                             lanes: every row access coalesces.  (The local cubics are hermite_build_kernel with its
//                             LANE_X accessor: h_i = x[i+1][l] - x[i][l].)
//   lane_axes_eval_kernel     BOTH evaluation entry points: one thread per output element, the flat index with lanes
//                             fastest (inverse_eval_kernel's mapping): stores coalesce, q[j] is a broadcast (ndi_interp1d_eval)
//                             or a coalesced load (ndi_interp1d_eval_lanewise), and the column reads x[mid * lanes + l] of
//                             neighbouring lanes coalesce while their searches agree
//   lane_axes_records_kernel  the record copy R[i][l] = {x, y, a, b} of the cubic class (row n-1: a = b = 0): after the
//                             search an element takes two aligned 16- / 32-byte loads instead of six element reads from
//                             four tables (DESIGN.md 4.23 has the measurement that decides where it is used)
#pragma once

namespace ndi {

// ---- creation: is every column strictly rising? -------------------------------------------------------------------------
// flags[l] != 0: some pair of column l is not strictly rising -- a tie, a fall, or a NaN on either side (n >= 2, so every
// knot is in a pair).  One thread walks INV_CHECK_RUN consecutive knots of one lane and publishes with at most one atomicOr.
template <class T>
__global__ __launch_bounds__(BLOCK) void lane_axes_check_kernel(const T* X, uint64_t n, uint64_t lanes, unsigned int* flags) {
  const uint64_t runs = (n + INV_CHECK_RUN - 1) / INV_CHECK_RUN, total = runs * lanes;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += step) {
    const uint64_t r = e / lanes, l = e - r * lanes;
    const uint64_t i0 = r * INV_CHECK_RUN;
    const uint64_t i1 = (n - i0 < INV_CHECK_RUN + 1) ? n : i0 + INV_CHECK_RUN + 1;   // the run's pairs reach into the next run
    unsigned int bits = 0;
    T prev = X[NDI_CHK(i0, n, BC_INTERVAL) * lanes + l];
    for (uint64_t i = i0 + 1; i < i1; ++i) {
      const T cur = X[NDI_CHK(i, n, BC_INTERVAL) * lanes + l];
      if (!(cur > prev)) bits |= 1u;
      prev = cur;
    }
    if (bits && (__atomic_load_n(&flags[l], __ATOMIC_RELAXED) & bits) != bits) atomicOr(&flags[l], bits);
  }
}

// ---- the CubicSpline build ------------------------------------------------------------------------------------------------
template <class T>
struct LaneAxesSplineArgs {
  const T* x;     // [n][lanes]
  const T* y;     // [n][lanes]
  T* ca;          // [n-1][lanes]
  T* cb;          // [n-1][lanes]
  T* mp;          // [n][lanes] scratch: the eliminated main diagonal
  T* rr;          // [n][lanes] scratch: the eliminated right-hand sides
  uint64_t n, lanes;
  int left_kind, right_kind;   // EndKind
  T left_val, right_val;
  int parabola;                // n == 3, NotAKnot on both ends: the parabola rows (cubic_spline.rs:569-596)
};

template <class T>
__global__ __launch_bounds__(64) void lane_axes_spline_kernel(LaneAxesSplineArgs<T> A) {
  const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= A.lanes) return;
  const uint64_t n = A.n, L = A.lanes;
  const T one = T(1), two = T(2), three = T(3);
  const T* x = A.x + l;
  const T* y = A.y + l;
  T* mp = A.mp + l;
  T* rr = A.rr + l;
  T* sa = A.ca + l;
  T* sb = A.cb + l;
  // the x-only scalars of the plan (make_spline_plan)
  const T dx0 = x[L] - x[0];
  const T dx1 = x[2 * L] - x[L];
  const T dxl = x[(n - 1) * L] - x[(n - 2) * L];    // dx_1 in the reference
  const T dxl2 = x[(n - 2) * L] - x[(n - 3) * L];   // dx_2
  const T dx0_sq = dx0 * dx0;
  const T dxl_sq = dxl * dxl;
  const T lval = A.left_val, rval = A.right_val;
  // ---- row 0 (:597-611; parabola :569-592)
  T mid_prev, up0, r_prev;
  {
    const T y0 = y[0], y1 = y[L], y2 = y[2 * L];
    if (A.parabola) {
      mid_prev = one;
      up0 = one;
      r_prev = ((y1 - y0) / dx0) * two;
    } else if (A.left_kind == END_NOT_A_KNOT) {
      mid_prev = dx1;
      const T d = x[2 * L] - x[0];
      up0 = d;
      const T tmp1 = (dx0 + two * d) * dx1;
      r_prev = (tmp1 * (y1 - y0) / dx0 + dx0_sq * (y2 - y1) / dx1) / d;
    } else if (A.left_kind == END_FIRST_DERIV) {
      mid_prev = one;
      up0 = T(0);
      r_prev = lval;
    } else {
      up0 = dx0;
      mid_prev = two * dx0;
      r_prev = three * (y1 - y0) - lval * dx0_sq / two;
    }
  }
  mp[0] = mid_prev;
  rr[0] = r_prev;
  // ---- rows 1 .. n-2: the diagonals (:440-451), the right-hand side (:456-471), the elimination (:690-700)
  T up_prev = up0;
  T xm = x[0], xc = x[L];
  T a0 = y[0], a1 = y[L];
  for (uint64_t i = 1; i + 1 < n; ++i) {
    const T xp = x[NDI_CHK(i + 1, n, BC_INTERVAL) * L], a2 = y[(i + 1) * L];
    const T dxn = xp - xc;
    const T dxn_1 = xc - xm;
    T low, mid, up, rhs;
    if (A.parabola) {
      low = dx1;
      mid = two * (dx0 + dx1);
      up = dx0;
      rhs = (((a2 - a1) / dx1) * dx0 + ((a1 - a0) / dx0) * dx1) * three;
    } else {
      up = dxn_1;
      mid = two * (dxn + dxn_1);
      low = dxn;
      rhs = three * (dxn * (a1 - a0) / dxn_1 + dxn_1 * (a2 - a1) / dxn);
    }
    const T w = low / mid_prev;
    const T prod = w * up_prev;
    const T midp = mid - prod;
    const T r = rhs - w * r_prev;
    mp[i * L] = midp;
    rr[i * L] = r;
    mid_prev = midp;
    up_prev = up;
    r_prev = r;
    xm = xc; xc = xp;
    a0 = a1; a1 = a2;
  }
  // ---- row n-1 (:634-670; parabola :595)
  T k_next;
  {
    const T ym = y[(n - 3) * L], yc = y[(n - 2) * L], yp = y[(n - 1) * L];
    T low, mid, rhs;
    if (A.parabola) {
      low = one;
      mid = one;
      rhs = ((yp - yc) / dxl) * two;
    } else if (A.right_kind == END_NOT_A_KNOT) {
      mid = dxl;   // sic: the reference uses dx_1 here (:635)
      const T d = x[(n - 1) * L] - x[(n - 3) * L];
      low = d;
      const T tmp1 = (two * d + dxl) * dxl2;
      rhs = (dxl_sq * (yc - ym) / dxl2 + tmp1 * (yp - yc) / dxl) / d;
    } else if (A.right_kind == END_FIRST_DERIV) {
      mid = one;
      low = T(0);
      rhs = rval;
    } else {
      mid = two * dxl;
      low = dxl;
      rhs = three * (yp - yc) + rval * dxl_sq / two;
    }
    const T w = low / mid_prev;
    const T prod = w * up_prev;
    const T mid_last = mid - prod;
    const T r_last = rhs - w * r_prev;
    k_next = r_last / mid_last;
  }
  // ---- back substitution (:702-721) fused with a / b (:350-365), rows n-2 .. 0
  T y_hi = y[(n - 1) * L], x_hi = x[(n - 1) * L];
  T x_lo = x[(n - 2) * L];
  for (uint64_t i = n - 1; i-- > 0;) {
    const uint64_t ii = NDI_CHK(i, n - 1, BC_INTERVAL);
    const T x_below = ii ? x[(ii - 1) * L] : T(0);
    const T up = ii ? x_lo - x_below : up0;   // up[i] = x[i] - x[i-1]; row 0: the boundary's
    const T k = (rr[ii * L] - up * k_next) / mp[ii * L];
    const T dxi = x_hi - x_lo;
    const T yl = y[ii * L];
    const T dy = y_hi - yl;
    sa[ii * L] = k * dxi - dy;
    sb[ii * L] = dy - k_next * dxi;
    k_next = k;
    y_hi = yl;
    x_hi = x_lo;
    x_lo = x_below;
  }
}

// ---- the record copy ------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(BLOCK) void lane_axes_records_kernel(const T* x, const T* y, const T* a, const T* b,
                                                                  LanewiseRecord<T, 4>* out, uint64_t n, uint64_t lanes) {
  const uint64_t total = n * lanes, tab = (n - 1) * lanes;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (uint64_t)gridDim.x * BLOCK) {
    LanewiseRecord<T, 4> r;
    r.v[0] = x[e];
    r.v[1] = y[e];
    r.v[2] = e < tab ? a[e] : T(0);
    r.v[3] = e < tab ? b[e] : T(0);
    out[e] = r;
  }
}

// ---- evaluation -----------------------------------------------------------------------------------------------------------
template <class T>
struct LaneAxesArgs {
  const T* x;       // [n][lanes]
  const T* y;       // [n][lanes]
  const T* a;       // [n-1][lanes] (cubic class)
  const T* b;
  const void* rec;  // LanewiseRecord<T, 4> [n][lanes] (REC), else unused
  const T* q;       // LANEQ: [rows][q_stride]; otherwise [rows]
  T* out;           // [rows][out_stride]
  const T* lo;      // LANEQ: [lanes] lane l's own range x[0][l] .. x[n-1][l]
  const T* hi;
  T Lo, Hi;         // !LANEQ: the range common to all lanes, max_l x[0][l] .. min_l x[n-1][l]
  LanewiseGeom G;
  uint64_t n;
  int mode;         // EX_NO / EX_YES
  int check;        // 1: the kernel publishes the lowest failing index itself; 0: first_fail holds the pre-pass's verdict
  unsigned long long* first_fail;   // LANEQ: a flat element index j * lanes + l; otherwise a query index j
};

// f_l(q): the search of the contract, then the point of the shared-axis lane-wise kernel on this lane's operands.
template <class T, int STRAT, bool REC>
__device__ __forceinline__ T lane_axes_element(const LaneAxesArgs<T>& A, T q, uint64_t l) {
  const uint64_t L = A.G.lanes, n = A.n;
  const T* c = A.x + l;
  uint64_t lo = 0, hi = n - 1;
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (c[NDI_CHK(mid, n, BC_INTERVAL) * L] <= q) lo = mid;
    else hi = mid;
  }
  const uint64_t i = NDI_CHK(lo, n - 1, BC_INTERVAL);
  const uint64_t at = i * L + l;
  T xl, xr, yl, yr, a = T(0), b = T(0);
  if constexpr (REC) {
    const LanewiseRecord<T, 4>* R = static_cast<const LanewiseRecord<T, 4>*>(A.rec);
    const LanewiseRecord<T, 4> r0 = R[at], r1 = R[at + L];
    xl = r0.v[0]; yl = r0.v[1]; a = r0.v[2]; b = r0.v[3];
    xr = r1.v[0]; yr = r1.v[1];
  } else {
    xl = A.x[at];
    xr = A.x[at + L];
    yl = A.y[at];
    yr = A.y[at + L];
    if (STRAT == ST_CUBIC) {
      a = A.a[at];
      b = A.b[at];
    }
  }
  RowCoef<T, STRAT> cf;
  if (STRAT == ST_CUBIC) {
    const T t = (q - xl) / (xr - xl);   // cubic_spline.rs:818
    const T one = T(1);
    cf.c0 = one - t;
    cf.c1 = t;
    cf.c2 = t * (one - t);
  } else {
    cf.c0 = xr - xl;
    cf.c1 = q - xl;
    cf.c2 = T(0);
  }
  return row_point<T, STRAT, T>(cf, yl, yr, a, b);
}

template <class T, int STRAT, bool LANEQ, bool REC>
__global__ __launch_bounds__(BLOCK) void lane_axes_eval_kernel(LaneAxesArgs<T> A) {
  const LanewiseGeom G = A.G;
  const uint64_t L = G.lanes;
  uint64_t rows = G.rows;
  if (!A.check) {   // rows at / after the first failure stay untouched
    if constexpr (LANEQ) {
      rows = lanewise_rows(G, A.first_fail, 0);
    } else {
      const unsigned long long f = *A.first_fail;
      if (f < rows) rows = f;
    }
  }
  const uint64_t total = rows * L;
  uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= total) return;
  LanewisePos p;
  p.start(G, e);
  for (; e < total; e += (uint64_t)gridDim.x * BLOCK, p.advance(G)) {
    const uint64_t j = NDI_CHK(p.j, G.rows, BC_QUERY), l = NDI_CHK(p.l, L, BC_LANE);
    const T q = LANEQ ? A.q[j * G.q_stride + l] : A.q[j];
    bool bad;
    if (A.mode != EX_NO) bad = !(q == q);
    else if constexpr (LANEQ) bad = !((A.lo[l] <= q) && (q <= A.hi[l]));
    else bad = !((A.Lo <= q) && (q <= A.Hi));
    if (bad) {   // (a NaN has no interval: the search is never run on one)
      if (A.check) atomicMin(A.first_fail, (unsigned long long)(LANEQ ? e : j));
      continue;
    }
    A.out[j * G.out_stride + l] = lane_axes_element<T, STRAT, REC>(A, q, l);
  }
}

}  // namespace ndi
